"""The inference-only surfel forward (gsr_surfel_forward_eval, _C.rasterize_gaussians_eval, gaussian_renderer.rasterize_eval) and
render_fast()'s use of it under torch.no_grad().  It compiles the training-only work of the forward out of the same kernels, so every
plane it returns must be the SAME BITS as the corresponding output of the training forward (gsr_surfel_forward_refl) for the same
inputs: each pixel's accumulation runs over the tile's list in the same order with the same arithmetic in both."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import HipSurfel, S

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- scenes
def _degenerate_transmats(n, W, H, seed):
    """Homographies whose splat plane contains the camera centre: k x l has a zero z component at every pixel, so every lane of every
    pair takes the forward's `unstable` (grazing) branch and the splat blends through the 2D low-pass filter alone."""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(0.5, 3.0, n), rs.uniform(0.5, 3.0, n)
    cx, cy = rs.uniform(0, W, n), rs.uniform(0, H, n)
    T = np.zeros((n, 9), np.float32)
    T[:, 0], T[:, 1], T[:, 2] = a, b, cx            # Tu
    T[:, 3], T[:, 4], T[:, 5] = 0.5 * a, 0.5 * b, cy   # Tv (parallel to Tu in its first two components)
    T[:, 8] = 1.0                                   # Tw = (0, 0, 1)
    return T


def _scene(P, W, H, seed=7, mu=-3.3, degree=3, colors=False, transmat=False, opaque=False, grazing=False, cull_frac=0.02, cam=None):
    cam = cam or S.look_at_camera(W, H, eye=(0.3, -0.2, -0.8), target=(0, 0, 5))
    sc = S.make_scene(P, "S", seed=seed, mu=mu, cull_frac=cull_frac)
    if opaque:
        sc["opacities"][:] = 1.0
    t = {k: torch.from_numpy(sc[k]).cuda() for k in ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")}
    t["colors"] = None
    t["transmat"] = None
    if colors:
        t["colors"] = torch.from_numpy(np.random.RandomState(seed).rand(P, 3).astype(np.float32)).cuda()
        t["shs"] = None
    if (transmat or grazing) and P > 0:
        kw = dict(bg=np.zeros(3, np.float32), means3D=sc["means3D"], opacities=sc["opacities"], viewmatrix=cam["viewmatrix"],
                  projmatrix=cam["projmatrix"], campos=cam["campos"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=H,
                  image_width=W, sh_degree=degree, shs=sc["shs"], refl_strengths=sc["refl_strengths"], scales=sc["scales"],
                  rotations=sc["rotations"], env_scope_mask=sc["env_scope_mask"])
        hs = HipSurfel(kw)
        T = hs.state("transMat")
        T[hs.radii.cpu().numpy() == 0] = np.eye(3, dtype=np.float32).reshape(-1)     # culled Gaussians never wrote their T
        if grazing:
            T[::2] = _degenerate_transmats(len(T[::2]), W, H, seed)
        t["transmat"] = torch.from_numpy(np.ascontiguousarray(T)).cuda()
        t["scales"] = t["rotations"] = None
    tex, fail = S.make_cubemap(16, 3, seed)
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}
    return dict(t=t, cam=cam, ct=ct, W=W, H=H, degree=degree, cubemap=torch.from_numpy(tex).cuda(), fail=torch.from_numpy(fail).cuda() + 0.25,
                bg=torch.tensor([0.1, 0.2, 0.3], device="cuda"))


def _args(s, prefiltered=False):
    """Positional arguments shared by _C.rasterize_gaussians (after env_scope_mask is inserted) and _C.rasterize_gaussians_eval."""
    t, ct, cam = s["t"], s["ct"], s["cam"]
    e = torch.empty(0, device="cuda")
    o = lambda x: e if x is None else x
    return [s["bg"], t["means3D"], o(t["colors"]), t["refl_strengths"], t["opacities"], o(t["scales"]), o(t["rotations"]), 1.0, o(t["transmat"]),
            ct["viewmatrix"], ct["projmatrix"], cam["tanfovx"], cam["tanfovy"], s["H"], s["W"], o(t["shs"]), s["degree"], ct["campos"],
            prefiltered, False]


def _refl(s):
    from gaussian_renderer import _cam_block
    return dict(cam=_cam_block(s["ct"]["viewmatrix"], (s["H"], s["W"], s["cam"]["K"]), s["ct"]["R"], s["ct"]["T"]), cubemap=s["cubemap"],
                fail_value=s["fail"])


def _compare(s, refl, prefiltered=False):
    from diff_surfel_rasterization import _C
    a = _args(s, prefiltered)
    r = _refl(s) if refl else None
    tr = _C.rasterize_gaussians(*a[:2], torch.empty(0, dtype=torch.bool, device="cuda"), *a[2:],
                                refl=None if r is None else dict(r, keys=False))
    ev = _C.rasterize_gaussians_eval(*a, refl=r)
    torch.cuda.synchronize()
    n_tr, color, others, radii, refl_map = tr[0], tr[1], tr[2], tr[3], tr[7]
    n_ev, e_color, e_alpha, e_normal, e_refl_map, e_radii = ev[:6]
    assert n_ev == n_tr
    assert torch.equal(e_radii, radii)
    assert torch.equal(e_color, color)
    assert torch.equal(e_alpha, others[1:2])
    assert torch.equal(e_refl_map, refl_map)
    if refl:
        assert e_normal is None
        for k, (x, y) in enumerate(zip(ev[6:9], tr[9:12])):
            assert torch.equal(x, y), ("final", "refl_color", "normal_world")[k]
    else:
        assert torch.equal(e_normal, others[2:5])
    return n_tr, others


# ------------------------------------------------------------------------------------------- bit identity with the training forward
@pytest.mark.parametrize("refl", [False, True])
@pytest.mark.parametrize("case", ["sh0", "sh1", "sh2", "sh3", "colors_precomp", "transmat", "prefiltered", "odd_size", "wide_grid", "opaque",
                                  "grazing", "empty"])
def test_eval_forward_is_bit_identical_to_the_training_forward(case, refl):
    prefiltered = False
    if case.startswith("sh"):
        s = _scene(6000, 320, 200, seed=11, degree=int(case[2]))
    elif case == "colors_precomp":
        s = _scene(6000, 320, 200, seed=12, colors=True)
    elif case == "transmat":
        s = _scene(6000, 320, 200, seed=13, transmat=True)
    elif case == "prefiltered":
        s = _scene(6000, 320, 200, seed=14, cull_frac=0.0)
        prefiltered = True
    elif case == "odd_size":
        s = _scene(40_000, 1001, 777, seed=15)
    elif case == "wide_grid":           # 257 x 4 tiles: beyond the 8-bit packed tile rectangles of the depth order
        s = _scene(20_000, 4100, 64, seed=16, cam=S.make_camera(4100, 64, fovy_deg=10.0))
    elif case == "opaque":              # every pixel saturates: the early exit
        s = _scene(40_000, 320, 200, seed=17, mu=-2.5, opaque=True)
    elif case == "grazing":
        s = _scene(6000, 320, 200, seed=18, grazing=True)
    else:
        s = _scene(0, 200, 120)
    n, others = _compare(s, refl, prefiltered)
    if case != "empty":
        assert n > 0 and float(others[1].max()) > 0.5          # the scene is really in view
    if case == "opaque":
        assert float((others[1] > 0.999).float().mean()) > 0.5


def test_eval_forward_is_bit_identical_at_c3():
    """The bench's C3 scene: 1 M surfels, 1920x1080, SH degree 3, reflection epilogue."""
    s = _scene(1_000_000, 1920, 1080, seed=1003, mu=-4.75, cam=S.make_camera(1920, 1080))
    tex, fail = S.make_cubemap(128, 3, 1003)
    s["cubemap"], s["fail"], s["bg"] = torch.from_numpy(tex).cuda(), torch.from_numpy(fail).cuda(), torch.zeros(3, device="cuda")
    n, _ = _compare(s, True)
    assert n > 1_000_000


# ------------------------------------------------------------------------------------------- every output is written
@pytest.mark.parametrize("refl", [False, True])
def test_eval_entry_writes_every_output_plane(refl):
    """Outputs pre-filled with NaN, image 1001x777 (partial tiles at the right and bottom edges): nothing NaN may remain."""
    import _gsr
    from _gsr import lib, ptr, stream_ptr
    s = _scene(20_000, 1001, 777, seed=21)
    t, ct, cam, W, H = s["t"], s["ct"], s["cam"], s["W"], s["H"]
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    color, alpha, normal, refl_map = nan(3, H, W), nan(H, W), (None if refl else nan(3, H, W)), nan(H, W)
    radii = torch.full((t["means3D"].shape[0],), -7, dtype=torch.int32, device="cuda")
    outs = [color, alpha, refl_map] + ([] if normal is None else [normal])
    desc = None
    if refl:
        r = _refl(s)
        L = int(s["cubemap"].shape[2])
        rgba = torch.empty(6 * L * L * 4, device="cuda")
        final, refl_color, nworld = nan(3, H, W), nan(3, H, W), nan(3, H, W)
        outs += [final, refl_color, nworld]
        desc = _gsr.ReflForward(ptr(r["cam"]), ptr(s["cubemap"]), ptr(s["fail"]), L, ptr(rgba), ptr(final), ptr(refl_color), ptr(nworld), None, None, 0, 0)
    ws = _gsr.Workspace(torch.device("cuda"))
    rc = lib.gsr_surfel_forward_eval(ws.cb, None, t["means3D"].shape[0], 3, 16, ptr(s["bg"]), W, H, ptr(t["means3D"]), ptr(t["shs"]), None,
                                     ptr(t["refl_strengths"]), ptr(t["opacities"]), ptr(t["scales"]), 1.0, ptr(t["rotations"]), None,
                                     ptr(ct["viewmatrix"]), ptr(ct["projmatrix"]), ptr(ct["campos"]), cam["tanfovx"], cam["tanfovy"], 0,
                                     ptr(color), ptr(alpha), ptr(normal), ptr(refl_map), ptr(radii),
                                     ctypes.byref(desc) if desc is not None else None, 0, stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    assert rc > 0, lib.gsr_last_error()
    for k, o in enumerate(outs):
        assert not torch.isnan(o).any(), k
    assert bool((radii >= 0).all())


# ------------------------------------------------------------------------------------------- render_fast dispatch
def _view(cam, W, H):
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}

    class View:
        FoVx, FoVy = cam["FoVx"], cam["FoVy"]
        image_width, image_height = W, H
        world_view_transform, full_proj_transform, camera_center = ct["viewmatrix"], ct["projmatrix"], ct["campos"]
        HWK, R, T = (H, W, cam["K"]), ct["R"], ct["T"]
        znear, zfar = cam["znear"], cam["zfar"]
    return View


class _Pipe:
    depth_ratio, compute_cov3D_python = 0.0, False


def _model(P, seed, L=32):
    from cubemapencoder import CubemapEncoder
    sc = S.make_scene(P, "S", seed=seed, mu=-3.3)
    tex, fail = S.make_cubemap(L, 3, seed)
    t = {k: torch.from_numpy(sc[k]).cuda().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")}
    env = CubemapEncoder(output_dim=3, resolution=L).cuda()
    with torch.no_grad():
        env.params["Cubemap_texture"].copy_(torch.from_numpy(tex))
        env.params["Cubemap_failv"].copy_(torch.from_numpy(fail) + 0.25)

    class PC:
        get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (t["means3D"], t["opacities"], t["scales"], t["rotations"],
                                                                                   t["shs"], t["refl_strengths"])
        active_sh_degree, get_envmap = 3, env
    return PC


def _raise(*a, **k):
    raise AssertionError("this path must not be taken here")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("initial_stage", [False, True])
def test_render_fast_under_no_grad_uses_the_eval_forward(monkeypatch, fused, initial_stage):
    import diff_surfel_rasterization
    import gaussian_renderer
    from gaussian_renderer import render, render_fast
    monkeypatch.setattr(gaussian_renderer, "FUSED_REFLECTION", fused)
    W, H = 400, 240
    View = _view(S.look_at_camera(W, H, eye=(0.4, -0.3, -1.0), target=(0, 0, 5)), W, H)
    PC = _model(30_000, 41)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    full = render(View, PC, _Pipe, bg, initial_stage=initial_stage)
    # no grad: the training forward must not run
    with monkeypatch.context() as m:
        m.setattr(diff_surfel_rasterization._C, "rasterize_gaussians", _raise)
        with torch.no_grad():
            fast = render_fast(View, PC, _Pipe, bg, initial_stage=initial_stage)
    keys = ("render", "rend_alpha", "rend_normal", "refl_strength_map") + (() if initial_stage else ("refl_color_map", "base_color_map"))
    assert set(fast.keys()) == set(keys)
    for k in keys:
        if k == "refl_strength_map" and initial_stage:
            continue                                    # render() does not return it in the initial stage
        assert torch.equal(fast[k], full[k]), k
    assert float(full["rend_alpha"].max()) > 0.5
    # grad mode on: the training forward, differentiable; the eval forward must not run
    with monkeypatch.context() as m:
        m.setattr(diff_surfel_rasterization._C, "rasterize_gaussians_eval", _raise)
        fast = render_fast(View, PC, _Pipe, bg, initial_stage=initial_stage)
        assert fast["render"].grad_fn is not None
        fast["render"].sum().backward()
    assert PC.get_opacity.grad is not None and torch.isfinite(PC.get_opacity.grad).all()
    assert torch.equal(fast["render"].detach(), full["render"].detach())


def test_rasterize_eval_refuses_inputs_that_require_grad():
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussian_renderer import rasterize_eval
    s = _scene(2000, 128, 96, seed=31)
    t, ct, cam = s["t"], s["ct"], s["cam"]
    rast = GaussianRasterizer(GaussianRasterizationSettings(image_height=96, image_width=128, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                                            bg=s["bg"], scale_modifier=1.0, viewmatrix=ct["viewmatrix"], projmatrix=ct["projmatrix"],
                                                            sh_degree=3, campos=ct["campos"], prefiltered=False, debug=False))
    kw = dict(shs=t["shs"], refl_strengths=t["refl_strengths"], scales=t["scales"], rotations=t["rotations"])
    opac = t["opacities"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="rasterize_eval has no backward"):
        rasterize_eval(rast, t["means3D"], opac, **kw)
    with torch.no_grad():
        out = rasterize_eval(rast, t["means3D"], opac, **kw)
    assert out["render"].shape == (3, 96, 128) and out["rend_alpha"].shape == (1, 96, 128) and out["rend_normal"].shape == (3, 96, 128)
    out2 = rasterize_eval(rast, t["means3D"], t["opacities"], **kw)    # grad mode on, nothing requires grad: allowed
    assert torch.equal(out["render"], out2["render"])
