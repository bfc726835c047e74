"""scene.GaussianModel and gsr_densification_stats_filter on the GPU.

The model is a facade: it holds one gsr_train.RawTrainState and one gsr_densify.DensifyStats and adds no arithmetic.  So the tests compare
it with the same state driven by hand (the recipe of INTEGRATION.md), bit for bit wherever the inputs are the same bits (synthetic
gradients), and within the spread of the rasterizer's float atomics where they come from a backward pass.  Shapes: P = 1031 (no multiple
of 4: every group's padding is live), SH degree 3, a cubemap of L = 8, images of 64 x 48, P = 0 and P = 1 at the edges."""
import types

import numpy as np
import pytest
import torch

import raw_step_ref as R
from poison import u32

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
P0, L0, W, H = 1031, 8, 64, 48
NAMES = ["means3D", "shs", "opacities", "scales", "rotations", "refl_strengths"]
STATS = ("xyz_gradient_accum", "denom", "accum_w", "denom_w", "max_radii2D")


def _opt(**over):
    """training_args: the reference's OptimizationParams as far as training_setup reads them."""
    from gsr_train import DEFAULT_LRS
    return types.SimpleNamespace(**dict(DEFAULT_LRS, percent_dense=0.01, **over))


def _lrs(opt):
    from gsr_train import DEFAULT_LRS
    return {k: getattr(opt, k) for k in DEFAULT_LRS}


def _bits(t):
    return u32(t.detach().cpu().numpy()).tobytes()


def _cloud(seed=3):
    """A point cloud whose 3-NN scales fall into three classes: a fine lattice (spacing 0.008: clone candidates under percent_dense *
    extent = 0.02), a coarse one (spacing 0.09: split candidates) and a few isolated points (scale around 0.6: big points at extent 2)."""
    rs = np.random.RandomState(seed)
    fine = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3) * 0.008 + [0.6, 0.0, 0.0]
    coarse = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3) * 0.09 - [0.7, 0.3, 0.3]
    far = np.array([[-1.2, 1.1, 0.9], [1.3, -1.0, 0.8], [0.1, 1.4, -1.1], [-1.3, -1.2, -0.9], [1.2, 1.2, 1.1], [0.0, -1.5, 1.2], [1.4, 0.1, -1.3]])
    pts = np.concatenate([fine, coarse, far]) + rs.randn(P0, 3) * 1e-4
    assert pts.shape == (P0, 3)
    return types.SimpleNamespace(points=pts.astype(np.float32), colors=rs.rand(P0, 3).astype(np.float32))


def _model_and_state(opt, scale=1.3, seed=11):
    """Side A: a GaussianModel from the cloud.  Side B: the same tensors wired by hand as INTEGRATION.md tells."""
    from gsr_densify import DensifyStats
    from gsr_init import init_from_point_cloud
    from gsr_train import RawTrainState
    from scene import GaussianModel
    pcd = _cloud()
    m = GaussianModel(3, init_cubemap_resol=L0)
    m.create_from_pcd(pcd, scale, generator=torch.Generator(device="cuda").manual_seed(seed))
    m.training_setup(opt)
    tensors = init_from_point_cloud(pcd.points, pcd.colors, sh_degree=3, cubemap_resolution=L0, generator=torch.Generator(device="cuda").manual_seed(seed))
    st = RawTrainState.from_activated(tensors, "cuda", spatial_lr_scale=scale, lrs=_lrs(opt))
    return m, st, DensifyStats(P0, "cuda")


def _leaves(m):
    """The tensors whose .grad the reference's backward fills, by state group."""
    env = m.get_envmap.params
    return dict(means3D=m.get_xyz, shs=m.get_features, opacities=m.get_opacity, scales=m.get_scaling, rotations=m.get_rotation,
                refl_strengths=m.get_refl, cubemap=env["Cubemap_texture"], fail=env["Cubemap_failv"])


def _carry_env_grads(old, new):
    """By hand what the model does for a successor state of a densification or a prune: the env group keeps its gradient, as the reference's does."""
    import _gsr
    from gsr_train import copy_groups
    _gsr.side_join(old.params.flat.device)
    copy_groups(((old.grads.flat, new.grads.flat),), old.params, new.params, ["cubemap", "fail"])
    return new


def _same_state(m, st, stats, where):
    a = m._state
    assert a.p["means3D"].shape[0] == st.p["means3D"].shape[0] == m.get_xyz.shape[0], where
    assert a.optimizer.step_count == st.optimizer.step_count, where
    for what, x, y in (("raw", a.params.flat, st.params.flat), ("exp_avg", a.optimizer.exp_avg, st.optimizer.exp_avg),
                       ("exp_avg_sq", a.optimizer.exp_avg_sq, st.optimizer.exp_avg_sq), ("activated", a.optimizer.act, st.optimizer.act),
                       ("statistics", m._stats.buf, stats.buf)):
        assert x.shape == y.shape and _bits(x) == _bits(y), (where, what)


# ------------------------------------------------------------------------------------------------- 1. the filter kernel
def _stats_filter(P, buf, g, f, w):
    import _gsr
    _gsr.check(_gsr.lib.gsr_densification_stats_filter(P, g.data_ptr(), f.view(torch.uint8).data_ptr(), w.data_ptr(), buf[0].data_ptr(), buf[1].data_ptr(),
                                                       buf[2].data_ptr(), buf[3].data_ptr(), _gsr.stream_ptr(buf.device)), "gsr_densification_stats_filter")


@pytest.mark.parametrize("P, pattern", [(P0, "third"), (P0, "none"), (P0, "all"), (1, "all"), (1, "none"), (513, "third")])
def test_filter_kernel_matches_the_radii_kernel_and_float64(P, pattern):
    """gsr_densification_stats_filter against gsr_densification_stats with radii = filter.to(int32): the four statistics bit for bit;
    the fifth row of the buffer (max_radii2D, which lies right behind them and is no argument) keeps a sentinel's bits; and against a
    float64 restatement at the tolerance of tests/test_gpu_densify.py::test_stats_kernel_matches_oracle_over_several_views (rtol 1e-6,
    atol 1e-12 on the gradient norms; the other three are float32 sums of exactly representable terms: equal)."""
    import _gsr
    rs = np.random.RandomState(100 + P)
    start = np.stack([rs.rand(P) * 1e-2, rs.randint(0, 9, P), rs.rand(P) * 3, rs.randint(0, 9, P)]).astype(np.float32)
    g = (rs.randn(P, 3) * 1e-3).astype(np.float32)
    w = (rs.rand(P) * (rs.rand(P) < 0.5) - 0.1 * (rs.rand(P) < 0.2)).astype(np.float32)      # zeros, negatives and positives
    f = {"third": np.arange(P) % 3 == 0, "none": np.zeros(P, bool), "all": np.ones(P, bool)}[pattern]
    sentinel = torch.from_numpy(np.full(P, 0x7fc0dead, np.uint32).view(np.float32))
    a = torch.cat([torch.from_numpy(start), sentinel[None]]).cuda()
    b = torch.from_numpy(start).cuda()
    b_max = torch.zeros(P, device="cuda")
    gt, wt, ft = torch.from_numpy(g).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(f).cuda()
    _stats_filter(P, a, gt, ft, wt)
    radii = ft.to(torch.int32)
    _gsr.check(_gsr.lib.gsr_densification_stats(P, gt.data_ptr(), radii.data_ptr(), wt.data_ptr(), b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(),
                                                b[3].data_ptr(), b_max.data_ptr(), _gsr.stream_ptr(b.device)), "gsr_densification_stats")
    torch.cuda.synchronize()
    assert _bits(a[:4]) == _bits(b)
    assert _bits(a[4]) == _bits(sentinel)
    got = a[:4].cpu().numpy()
    norm = np.sqrt((g.astype(np.float64) ** 2).sum(axis=1))
    np.testing.assert_allclose(got[0], start[0].astype(np.float64) + np.where(f, norm, 0.0), rtol=1e-6, atol=1e-12)
    np.testing.assert_array_equal(got[1], start[1] + f.astype(np.float32))
    np.testing.assert_array_equal(got[2], np.where(w > 0, start[2] + w, start[2]))
    np.testing.assert_array_equal(got[3], start[3] + (w > 0).astype(np.float32))
    off = ~f
    assert u32(got[0][off]).tobytes() == u32(start[0][off]).tobytes()          # rows with the filter off keep their bits


def test_filter_entry_takes_no_rows_as_a_no_op():
    import _gsr
    assert _gsr.lib.gsr_densification_stats_filter(0, None, None, None, None, None, None, None, _gsr.stream_ptr(torch.device("cuda", 0))) == 0


# ------------------------------------------------------------------------------------------------- 2. views, not copies
def test_getters_are_views_of_the_state():
    opt = _opt()
    m, _, _ = _model_and_state(opt)
    st, stats = m._state, m._stats
    assert type(st).__name__ == "RawTrainState" and type(stats).__name__ == "DensifyStats" and m.get_xyz.shape == (P0, 3)
    for getter, view in (("get_xyz", st.p["means3D"]), ("get_features", st.p["shs"]), ("get_opacity", st.a["opacities"]), ("get_scaling", st.a["scales"]),
                         ("get_rotation", st.a["rotations"]), ("get_refl", st.a["refl_strengths"]), ("_xyz", st.p["means3D"]),
                         ("_opacity", st.p["opacities"]), ("_scaling", st.p["scales"]), ("_rotation", st.p["rotations"]),
                         ("_refl_strength", st.p["refl_strengths"])):
        assert getattr(m, getter) is view, getter
        assert getattr(m, getter).data_ptr() == view.data_ptr() and getattr(m, getter).shape == view.shape, getter
    assert m.get_features.shape == (P0, 16, 3) and m._features_dc.shape == (P0, 1, 3) and m._features_rest.shape == (P0, 15, 3)
    assert m._features_dc.data_ptr() == st.p["shs"].data_ptr() and m._features_rest.data_ptr() == st.p["shs"].data_ptr() + 12
    assert m._features_dc.stride() == m._features_rest.stride() == (48, 3, 1)
    a, _ = st.params.slices["opacities"]
    assert m.get_opacity.grad.data_ptr() == st.grads.flat.data_ptr() + 4 * a
    for k, leaf in _leaves(m).items():
        assert leaf.is_leaf and leaf.requires_grad and leaf.grad.data_ptr() == st.grads.view(k).data_ptr(), k
    env = m.get_envmap
    assert env is not None and m.env_map.params["Cubemap_texture"].data_ptr() == st.p["cubemap"].data_ptr()
    assert env.params["Cubemap_failv"].data_ptr() == st.p["fail"].data_ptr()
    assert env(torch.nn.functional.normalize(torch.randn(5, 3, device="cuda"))).shape == (5, 3)
    for row, name in enumerate(STATS[:4]):
        assert getattr(m, name).shape == (P0, 1) and getattr(m, name).data_ptr() == stats.buf[row].data_ptr(), name
    assert m.max_radii2D.shape == (P0,) and m.max_radii2D.data_ptr() == stats.buf[4].data_ptr()
    # the reference's line (train.py:243)
    radii = (torch.arange(P0, device="cuda") % 5).to(torch.int32)
    visibility_filter = radii > 0
    m.max_radii2D[visibility_filter] = torch.max(m.max_radii2D[visibility_filter], radii[visibility_filter])
    assert torch.equal(stats.buf[4], radii.float())
    # the optimizer's groups
    groups = m.optimizer.param_groups
    assert [g["name"] for g in groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "refl", "env"]
    assert [len(g["params"]) for g in groups] == [1, 1, 1, 1, 1, 1, 1, 2]
    assert groups[0]["lr"] == opt.position_lr_init * 1.3 and groups[2]["lr"] == opt.feature_lr / 20.0 and groups[7]["lr"] == opt.envmap_cubemap_lr
    assert groups[0]["params"][0] is m._xyz and groups[3]["params"][0] is m._opacity
    from cubemapencoder import CubemapEncoder
    order = [n.split(".")[-1] for n, _ in CubemapEncoder(output_dim=3, resolution=2).named_parameters()]
    assert [p.data_ptr() for p in groups[7]["params"]] == [env.params[n].data_ptr() for n in order]
    # get_covariance: the splat-to-world matrices in torch ops
    cov = m.get_covariance(0.5).detach()
    assert cov.shape == (P0, 4, 4) and torch.equal(cov[:, 3, :3], m.get_xyz) and bool((cov[:, :, 3] == torch.tensor([0.0, 0, 0, 1], device="cuda")).all())
    normal = torch.nn.functional.normalize(m._rotation.detach().double())
    w_, x_, y_, z_ = normal.unbind(1)
    n3 = torch.stack([2 * (x_ * z_ + w_ * y_), 2 * (y_ * z_ - w_ * x_), 1 - 2 * (x_ * x_ + y_ * y_)], dim=1)
    assert float((cov[:, 2, :3].double() - n3).abs().max()) < 1e-6
    assert float((cov[:, 0, :3].norm(dim=1) - 0.5 * m.get_scaling.detach()[:, 0]).abs().max()) < 1e-6 * float(m.get_scaling.detach().max()) + 1e-9


# ------------------------------------------------------------------------------------------------- 3. the facade adds no arithmetic
def test_twelve_iterations_of_the_reference_s_calls_equal_the_hand_wired_state_bit_for_bit():
    """Side A: a GaussianModel driven through the reference's method names only.  Side B: RawTrainState + DensifyStats wired by hand.
    Gradients, filters, weights and noise come from seeded generators (a rasterizer's backward sums with float atomics and does not
    repeat its bits).  Order inside an iteration: the reference's (train.py:120-306): learning rate, backward, double_env_map, freeze_xyz,
    statistics, densification, resets, colour sabotage, optimizer step."""
    import gsr_envmap
    from gsr_densify import densify_and_prune, prune_points
    opt = _opt()
    m, st, stats = _model_and_state(opt)
    _same_state(m, st, stats, "start")
    gen = torch.Generator().manual_seed(77)
    held = list(m.optimizer.param_groups)          # a caller may keep the group dicts, as with torch.optim.Adam
    mean, extent, max_grad = torch.zeros(3), 2.0, 0.0002
    infos = []
    for it in range(1, 13):
        # ---- learning rate
        lr_a, lr_b = m.update_learning_rate(it), st.update_learning_rate(it)
        assert lr_a == lr_b
        if it == 2:
            m.set_opacity_lr(0.0)
            st.set_lr("opacities", 0.0)
        if it == 3:
            m.set_opacity_lr(opt.opacity_lr)
            st.set_lr("opacities", opt.opacity_lr)
        # ---- "backward": the same seeded dL/d(activated) into both gradient buffers
        for k, leaf in _leaves(m).items():
            g = (torch.randn(leaf.shape, generator=gen) * 1e-3).cuda()
            leaf.grad.copy_(g)
            st.grads.view(k).copy_(g)
        if it == 6:
            m.double_env_map()
            st = gsr_envmap.double_env_map(st)
            assert m.env_map_resol == 2 * L0 and m.get_envmap.params["Cubemap_texture"].shape == (6, 3, 2 * L0, 2 * L0)
        if it >= 11:
            m.freeze_xyz()
            st.freeze(("means3D", "rotations"))
        # ---- statistics
        P = m.get_xyz.shape[0]
        viewspace = torch.zeros(P, 3, device="cuda", requires_grad=True)
        scale = torch.rand(P, 1, generator=gen) * 2.0
        viewspace.grad = (torch.randn(P, 3, generator=gen) * 2e-4 * scale).cuda()
        radii = (torch.randint(1, 40, (P,), generator=gen) * (torch.rand(P, generator=gen) < 0.6)).to(torch.int32).cuda()
        weights = (torch.rand(P, generator=gen) * 0.04 * (torch.rand(P, generator=gen) < 0.7)).cuda()
        visibility_filter = radii > 0
        if it % 2:        # the reference's two lines (train.py:243-245)
            m.max_radii2D[visibility_filter] = torch.max(m.max_radii2D[visibility_filter], radii[visibility_filter])
            m.add_densification_stats(viewspace, visibility_filter, weights)
        else:             # the fused form
            m.add_densification_stats(viewspace, visibility_filter, weights, radii=radii)
        stats.update(viewspace.grad, radii, weights)
        # ---- densification
        if it in (4, 8):
            size_threshold = 20 if it == 8 else None
            noise = torch.randn(2 * P, 2, generator=gen).cuda()
            info = m.densify_and_prune(max_grad, 0.05, mean, extent, size_threshold, noise=noise)
            new, stats, info_b = densify_and_prune(st, stats, max_grad, 0.05, mean, extent, size_threshold, percent_dense=opt.percent_dense, noise=noise,
                                                   plan="device")
            st = _carry_env_grads(st, new)
            assert info == info_b
            assert bool(m._state.grads.view("cubemap").any()) and not m._state.grads.view("means3D").any()      # the env group keeps its gradient
            infos.append(info)
        if it == 5:
            m.reset_opacity()
            st.reset_opacity()
        if it == 7:       # the normal-propagation block (train.py:265-281)
            opacity_old = m.get_opacity
            opac_mask = (opacity_old > 0.9).flatten()
            m.reset_opacity(reset_value=0.9, exclusive_msk=opac_mask)
            refl = m.get_refl
            scale_mask = (refl < 0.02).flatten()
            m.reset_scale(enlarge_scale=1.5, exclusive_msk=scale_mask)
            m.reset_refl()
            m.set_opacity_lr(0.0)
            st.reset_opacity(reset_value=0.9, exclusive_msk=(st.a["opacities"] > 0.9).flatten())
            st.reset_scale(enlarge_scale=1.5, exclusive_msk=(st.a["refl_strengths"] < 0.02).flatten())
            st.reset_refl(1e-3)
            st.set_lr("opacities", 0.0)
        if it == 9:       # the colour sabotage (train.py:283-290), and the opacity rate back (:260-261)
            noise = torch.rand(P, 1, 3, generator=gen).cuda()
            m.dist_color(exclusive_msk=(m.get_refl > 0.1).flatten(), noise=noise)
            st.dist_color(exclusive_msk=(st.a["refl_strengths"] > 0.1).flatten(), noise=noise)
            held[3]["lr"] = opt.opacity_lr           # (written through a dict taken before two densifications and an env-map resize)
            st.set_lr("opacities", opt.opacity_lr)
        if it == 10:
            mask = (torch.rand(P, generator=gen) < 0.1).cuda()
            m.prune_points(mask)
            new, stats, info_b = prune_points(st, mask, stats)
            st = _carry_env_grads(st, new)
            assert info_b["pruned"] == int(mask.sum()) > 0 and m.get_xyz.shape[0] == P - info_b["pruned"]
        # ---- optimizer step
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        st.optimizer.step()
        st.grads.zero_()
        torch.cuda.synchronize()
        assert m.optimizer.param_groups[0]["params"][0] is m._xyz and m.get_opacity.grad.data_ptr() == m._state.grads.view("opacities").data_ptr()
        assert not m._state.grads.flat.any()
        _same_state(m, st, stats, f"iteration {it}")
    assert all(a is b for a, b in zip(held, m.optimizer.param_groups)) and held[0]["params"][0] is m._xyz
    print("densifications:", infos)
    for info in infos:       # neither passes on empty selections
        assert info["pruned_by_weight"] >= 1 and info["cloned"] >= 1 and info["split"] >= 1, info
    assert infos[0]["pruned_big"] == 0 and infos[1]["pruned_big"] >= 1, infos
    assert m.get_xyz.shape[0] != P0 and m._state.optimizer.step_count == 12 and m._state.optimizer.frozen == {"means3D", "rotations"}


# ------------------------------------------------------------------------------------------------- 4. plain autograd end to end
def _view_and_scene(tmp_path, P=P0, seed=13, mu=-2.2):
    """The synthetic scene of the train tests (gsr_synth), written as the reference's PLY + .map with RAW values; its camera as a view."""
    import gsr_synth as S
    from gsr_train import inverse_sigmoid
    from scene.ply_io import save_ply
    sc = S.make_scene(P, "S", seed=seed, mu=mu)
    tex, fail = S.make_cubemap(L0, 3, seed)
    cam = S.make_camera(W, H)
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}

    class View:
        FoVx, FoVy = 2 * np.arctan(cam["tanfovx"]), 2 * np.arctan(cam["tanfovy"])
        image_width, image_height = W, H
        world_view_transform, full_proj_transform, camera_center = ct["viewmatrix"], ct["projmatrix"], ct["campos"]
        HWK, R, T = (H, W, cam["K"]), ct["R"], ct["T"]
        znear, zfar = 0.01, 100.0

    t = {k: torch.from_numpy(sc[k]) for k in NAMES}

    def write(name, shs, opacities):
        path = str(tmp_path / name)
        save_ply(path, t["means3D"], shs, inverse_sigmoid(opacities), inverse_sigmoid(t["refl_strengths"]), torch.log(t["scales"]), t["rotations"],
                 cubemap=tex, fail_value=fail)
        return path
    g = torch.Generator().manual_seed(1)
    truth = write("truth.ply", t["shs"], t["opacities"])
    start = write("start.ply", t["shs"] + 0.3 * torch.randn(t["shs"].shape, generator=g), t["opacities"] * 0.7)
    return View, truth, start


def _state_from_ply(path, opt=None, scale=1.0):
    """Side B: scene.ply_io.load_ply wired by hand."""
    from gsr_train import RawTrainState
    from scene.ply_io import load_ply
    data = load_ply(path, 3)
    return RawTrainState({k: torch.tensor(data[k]) for k in NAMES + ["cubemap", "fail"]}, "cuda", spatial_lr_scale=scale,
                         lrs=None if opt is None else _lrs(opt))


def test_the_reference_s_iteration_body_under_plain_autograd(tmp_path):
    """train.py:143-306 against render(), no sinks: six iterations with one densification.  Everything stays finite, the loss falls, and the
    parameters agree with the hand-wired, sink-free state within 4 x the spread two runs of that hand-wired state show between themselves
    (the rasterizer's backward sums with float atomics) + 2 ulp of the group's largest value; the spread is measured on side B alone.
    Then the same body runs with the model's sinks bound to the pipe.

    The densification stands where the reference has it, between backward() and optimizer.step().  The successor state it returns starts
    with zero gradient slots; the model, and side B by hand, carry the env group's two slots over, as the reference's env group keeps its
    .grad through a densification.  Without that the step would take the cubemap over a zero gradient: the second moment loses that
    iteration's term, and texels whose gradient is the small residual of cancelling pixel contributions (3e-7 with 1e-10 of run-to-run
    noise from the rasterizer's atomics upstream) then take steps lr * (1 - beta1) * dg / (bc1 * sqrt(v)) that turn that noise into 2e-6
    of texture, five to twenty times the spread two runs usually show."""
    from gaussian_renderer import render
    from gsr_densify import DensifyStats, densify_and_prune
    from scene import GaussianModel
    from utils.loss_utils import l1_loss, ssim
    View, truth, start = _view_and_scene(tmp_path)
    opt = _opt()
    opt.lambda_dssim, opt.lambda_normal = 0.2, 0.05
    bg = torch.zeros(3, device="cuda")
    mean, extent = torch.zeros(3), 5.0

    class Pipe:
        depth_ratio, compute_cov3D_python = 0.0, False

    truth_model = GaussianModel(3)
    truth_model.load_ply(truth)
    assert truth_model.optimizer is None and truth_model.env_map_resol == L0 and truth_model.active_sh_degree == 3
    with torch.no_grad():
        gt_image = render(View, truth_model, Pipe, bg)["render"].detach().clone()
    assert float(gt_image.abs().max()) > 0

    def loss_of(render_pkg):
        image = render_pkg["render"]
        Ll1 = l1_loss(image, gt_image)
        loss = (1.0 - opt.lambda_dssim) * Ll1 + opt.lambda_dssim * (1.0 - ssim(image, gt_image))
        normal_error = (1 - (render_pkg["rend_normal"] * render_pkg["surf_normal"]).sum(dim=0))[None]
        return loss + opt.lambda_normal * normal_error.mean()

    def noise_for(it):
        return torch.randn(4096, 2, generator=torch.Generator().manual_seed(it)).cuda()

    threshold = {}

    def grad_threshold(xyz_gradient_accum, denom):
        """The scene is tiny and has one view: the reference's 0.0002 would clone or split most of it at once.  The densification takes the
        three rows in a thousand with the largest mean view-space gradient instead (each split replaces one of the most visible surfels by
        two sampled children, which moves the image more than a step of the optimizer does); the number is formed once and serves every run."""
        if not threshold:
            mean_grad = torch.nan_to_num(xyz_gradient_accum / denom, nan=0.0).flatten()
            threshold["max_grad"] = float(torch.quantile(mean_grad, 0.997))
        return threshold["max_grad"]

    def body(gaussians, pipe, iteration):
        """The reference's iteration, its gaussians.* lines unchanged."""
        gaussians.update_learning_rate(iteration)
        render_pkg = render(View, gaussians, pipe, bg)
        loss = loss_of(render_pkg)
        loss.backward()
        with torch.no_grad():
            viewspace_point_tensor, visibility_filter, radii = render_pkg["viewspace_points"], render_pkg["visibility_filter"], render_pkg["radii"]
            gaussians.max_radii2D[visibility_filter] = torch.max(gaussians.max_radii2D[visibility_filter], radii[visibility_filter])
            render_weight = render_pkg["gaussian_weights"]
            gaussians.add_densification_stats(viewspace_point_tensor, visibility_filter, render_weight)
            if iteration == 2:
                info = gaussians.densify_and_prune(grad_threshold(gaussians.xyz_gradient_accum, gaussians.denom), 0.05, mean, extent, None,
                                                   noise=noise_for(iteration))
                print("densification:", info)
                assert info["cloned"] + info["split"] >= 1 and info["after"] != info["before"], info
            gaussians.optimizer.step()
            gaussians.optimizer.zero_grad(set_to_none=True)
        return float(loss.detach())

    def side_b():
        st = _state_from_ply(start, opt)
        stats = DensifyStats(P0, "cuda")
        for iteration in range(1, 7):
            st.update_learning_rate(iteration)
            render_pkg = render(View, st.model(3), Pipe, bg)
            loss_of(render_pkg).backward()
            stats.update(render_pkg["viewspace_points"].grad, render_pkg["radii"], render_pkg["gaussian_weights"])
            if iteration == 2:
                new, stats, _ = densify_and_prune(st, stats, threshold["max_grad"], 0.05, mean, extent, None, percent_dense=opt.percent_dense,
                                                  noise=noise_for(iteration), plan="device")
                st = _carry_env_grads(st, new)
            st.optimizer.step()
            st.grads.zero_()
        return st

    gaussians = GaussianModel(3)
    gaussians.load_ply(start)
    gaussians.spatial_lr_scale = 1.0
    gaussians.training_setup(opt)
    losses = [body(gaussians, Pipe, iteration) for iteration in range(1, 7)]
    print("losses", losses, "points", gaussians.get_xyz.shape[0])
    assert np.isfinite(losses).all() and bool(torch.isfinite(gaussians._state.params.flat).all()) and bool(torch.isfinite(gaussians._stats.buf).all())
    assert losses[-1] < losses[0], losses
    b1, b2 = side_b(), side_b()
    P1 = gaussians.get_xyz.shape[0]
    assert P1 == b1.p["means3D"].shape[0] == b2.p["means3D"].shape[0], "a densification decision fell on a threshold: the runs took different rows"
    for k in b1.params.names:
        ref = b1.p[k].detach().double()
        spread = float((b2.p[k].detach().double() - ref).abs().max())
        err = float((gaussians._state.p[k].detach().double() - ref).abs().max())
        bound = 4 * spread + 2 * ULP * float(ref.abs().max())
        print(f"{k:15s} model against hand-wired {err:.3e}  spread of two hand-wired runs {spread:.3e}  bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    # ---- the same body with the sinks bound
    pipe = types.SimpleNamespace(depth_ratio=0.0, compute_cov3D_python=False, gsr_accumulate=False)
    gaussians.bind(pipe)
    before = gaussians._state.params.flat.clone()
    for iteration in (7, 8):
        assert pipe.gsr_grad_sink["means3D"].data_ptr() == gaussians._xyz.grad.data_ptr()
        assert pipe.gsr_reflection_grad_sink["cubemap"].data_ptr() == gaussians._state.grads.view("cubemap").data_ptr() and pipe.gsr_accumulate is False
        losses.append(body(gaussians, pipe, iteration))
    assert np.isfinite(losses).all() and bool(torch.isfinite(gaussians._state.params.flat).all())
    assert bool((gaussians._state.params.flat != before).any()) and losses[-1] < losses[0], losses
    # a successor state takes the binding along
    gaussians.prune_points(torch.arange(P1, device="cuda") % 7 == 0)
    assert pipe.gsr_grad_sink["means3D"].data_ptr() == gaussians._xyz.grad.data_ptr() and gaussians._xyz.shape[0] < P1


# ------------------------------------------------------------------------------------------------- 5. checkpoint
def _synthetic_steps(m, gen, n):
    for _ in range(n):
        grads = {}
        for k, leaf in _leaves(m).items():
            grads[k] = (torch.randn(leaf.shape, generator=gen) * 1e-3).cuda()
            leaf.grad.copy_(grads[k])
        m.optimizer.step()
        torch.cuda.synchronize()
    return grads


def test_checkpoint_capture_restore_and_the_torch_adam_layout(tmp_path):
    from scene import GaussianModel
    opt = _opt()
    m, _, _ = _model_and_state(opt)
    gen = torch.Generator().manual_seed(5)
    m.update_learning_rate(3)
    _synthetic_steps(m, gen, 2)
    m.optimizer.zero_grad()
    m.xyz_gradient_accum[::3] += 0.25
    m.denom[::3] += 1
    m.max_radii2D[::5] = 7.0
    m.oneupSHdegree()
    captured = m.capture()
    assert len(captured) == 14 and captured[0] == 1 and captured[12] == 1.3 and captured[13] == L0
    for i, t in enumerate((m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity, m._refl_strength, m.max_radii2D,
                           m.xyz_gradient_accum, m.denom)):
        assert captured[1 + i].data_ptr() == t.data_ptr() and captured[1 + i].shape == t.shape, i
    sd = captured[11]
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(9))
    assert [g["name"] for g in sd["param_groups"]] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "refl", "env"]
    assert [g["params"] for g in sd["param_groups"]] == [[0], [1], [2], [3], [4], [5], [6], [7, 8]]
    assert all({"lr", "betas", "eps", "name", "params"} <= set(g) for g in sd["param_groups"])
    nine = [m._xyz, m._features_dc, m._features_rest, m._opacity, m._scaling, m._rotation, m._refl_strength] + m.optimizer.param_groups[7]["params"]
    moments = {m._state.optimizer.exp_avg.data_ptr(), m._state.optimizer.exp_avg_sq.data_ptr()}
    for i, p in enumerate(nine):
        e = sd["state"][i]
        assert int(e["step"]) == 2 and e["exp_avg"].shape == e["exp_avg_sq"].shape == p.shape, i
        assert e["exp_avg"].is_contiguous() and e["exp_avg"].untyped_storage().data_ptr() not in moments, i
    assert bool(sd["state"][1]["exp_avg"].any()) and bool(sd["state"][2]["exp_avg_sq"].any())
    # ---- load_state_dict(state_dict()) is the identity on the flat moments
    o = m._state.optimizer
    before = (o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count, dict(o.groups))
    m.optimizer.load_state_dict(m.optimizer.state_dict())
    assert _bits(o.exp_avg) == _bits(before[0]) and _bits(o.exp_avg_sq) == _bits(before[1]) and o.step_count == before[2] and o.groups == before[3]
    # ---- a second model restored from the tuple takes the next step as the first does
    path = str(tmp_path / "point_cloud.ply")
    m.save_ply(path)
    m2 = GaussianModel(3)
    m2.load_ply(path)            # (the tuple carries no environment map, in the reference neither: the model restores into the one it has)
    m2.restore(captured, opt)
    assert m2.active_sh_degree == 1 and m2.spatial_lr_scale == 1.3 and m2.percent_dense == opt.percent_dense and m2.env_map_resol == L0
    assert _bits(m2._stats.buf[[0, 1, 4]]) == _bits(m._stats.buf[[0, 1, 4]]) and not m2._stats.buf[[2, 3]].any()
    assert _bits(m2._state.params.flat) == _bits(m._state.params.flat)
    gen_a, gen_b = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    raw_before = m._state.params.flat.detach().cpu().numpy().copy()
    m_before, v_before = o.exp_avg.cpu().numpy().copy(), o.exp_avg_sq.cpu().numpy().copy()
    act_before = o.act.cpu().numpy().copy()
    grads = _synthetic_steps(m, gen_a, 1)
    _synthetic_steps(m2, gen_b, 1)
    for what, x, y in (("raw", m._state.params.flat, m2._state.params.flat), ("exp_avg", o.exp_avg, m2._state.optimizer.exp_avg),
                       ("exp_avg_sq", o.exp_avg_sq, m2._state.optimizer.exp_avg_sq), ("activated", o.act, m2._state.optimizer.act)):
        assert _bits(x) == _bits(y), what
    assert m2._state.optimizer.step_count == o.step_count == 3
    # ---- the state dict in a real torch.optim.Adam, built as the reference's training_setup builds it, takes the same step
    params = m._state.params
    raw0 = torch.from_numpy(raw_before).cuda()
    shs0 = params.view_of(raw0, "shs")
    order = m.optimizer._env
    clones = dict(xyz=[params.view_of(raw0, "means3D")], f_dc=[shs0[:, :1]], f_rest=[shs0[:, 1:]], opacity=[params.view_of(raw0, "opacities")],
                  scaling=[params.view_of(raw0, "scales")], rotation=[params.view_of(raw0, "rotations")], refl=[params.view_of(raw0, "refl_strengths")],
                  env=[params.view_of(raw0, k) for k in order])
    clones = {n: [t.clone().requires_grad_(True) for t in ts] for n, ts in clones.items()}
    adam = torch.optim.Adam([dict(params=clones[g["name"]], lr=g["lr"], name=g["name"]) for g in sd["param_groups"]], lr=0.0, eps=1e-15)
    adam.load_state_dict(sd)
    B1, B2 = R.f32(0.9), R.f32(0.999)
    for g in adam.param_groups:      # every chain steps with the constants the C entry's float arguments carry (tests/test_gpu_raw_step.py)
        g["lr"], g["betas"] = R.f32(g["lr"]), (B1, B2)
    activated = dict(xyz=[lambda r: r], f_dc=[lambda r: r], f_rest=[lambda r: r], opacity=[torch.sigmoid], scaling=[torch.exp],
                     rotation=[torch.nn.functional.normalize], refl=[torch.sigmoid], env=[lambda r: r, lambda r: r])
    upstream = dict(xyz=[grads["means3D"]], f_dc=[grads["shs"][:, :1]], f_rest=[grads["shs"][:, 1:]], opacity=[grads["opacities"]],
                    scaling=[grads["scales"]], rotation=[grads["rotations"]], refl=[grads["refl_strengths"]], env=[grads[k] for k in order])
    for n in clones:
        for leaf, act, up in zip(clones[n], activated[n], upstream[n]):
            act(leaf).backward(up)
    adam.step()
    torch.cuda.synchronize()
    # the float64 restatement of the same step, and the bound of tests/test_gpu_raw_step.py: 4 x (torch float32 against it) + 2 ulp
    segs, n_act = R.segments_of(params, m._state.optimizer.groups)
    gflat = np.zeros(params.total, np.float32)
    for k in params.names:
        a, b = params.slices[k]
        gflat[a:b] = grads[k].cpu().numpy().reshape(-1)
    ref = R.step(raw_before, gflat, m_before, v_before, act_before, segs, 3, betas=(B1, B2))
    exempt = R.rotation_exempt(params, ref["raw_grad"], gflat)
    c32 = {q: np.zeros(params.total) for q in ("raw", "m", "v")}
    P = params.shapes["shs"][0]
    place = dict(xyz=[("means3D", None)], f_dc=[("shs", slice(0, 1))], f_rest=[("shs", slice(1, None))], opacity=[("opacities", None)],
                 scaling=[("scales", None)], rotation=[("rotations", None)], refl=[("refl_strengths", None)], env=[(k, None) for k in order])
    for n in clones:
        for leaf, (k, rows) in zip(clones[n], place[n]):
            a, b = params.slices[k]
            for q, t in (("raw", leaf.detach()), ("m", adam.state[leaf]["exp_avg"]), ("v", adam.state[leaf]["exp_avg_sq"])):
                dst = c32[q][a:b].reshape(params.shapes[k])
                if rows is None:
                    dst[...] = t.cpu().numpy()
                else:
                    dst[:, rows] = t.cpu().numpy()
    got = dict(raw=m._state.params.flat.detach().cpu().numpy().astype(np.float64), m=o.exp_avg.cpu().numpy().astype(np.float64),
               v=o.exp_avg_sq.cpu().numpy().astype(np.float64))
    for k in params.names:
        a, b = params.slices[k]
        idx = np.arange(a, b)[~exempt[a:b]]
        for q in ("raw", "m", "v"):
            e32 = float(np.abs(c32[q][idx] - ref[q][idx]).max())
            err = float(np.abs(got[q][idx] - ref[q][idx]).max())
            bound = 4.0 * e32 + 2.0 * ULP * float(np.abs(ref[q][idx]).max())
            print(f"{k:15s} {q:3s} model {err:.3e}  torch.optim.Adam float32 {e32:.3e}  bound {bound:.3e}")
            assert err <= bound, (k, q, err, bound)
        assert float(np.abs(got["raw"][idx] - raw_before[idx]).max()) > 0 or k == "fail", k
    assert int(exempt.sum()) <= 2


# ------------------------------------------------------------------------------------------------- 6. PLY
def test_ply_round_trip_and_render_fast_of_a_loaded_model(tmp_path):
    from gaussian_renderer import render_fast
    from scene import GaussianModel
    from scene.ply_io import save_ply
    View, truth, _ = _view_and_scene(tmp_path)
    hand = _state_from_ply(truth)
    a = GaussianModel(3, init_cubemap_resol=4)
    a.load_ply(truth)                                   # a file scene.ply_io.save_ply wrote directly
    assert a.optimizer is None and a.env_map_resol == L0 and a.active_sh_degree == a.max_sh_degree == 3
    assert _bits(a._state.params.flat) == _bits(hand.params.flat) and _bits(a._state.optimizer.act) == _bits(hand.optimizer.act)
    a.training_setup(_opt())
    _synthetic_steps(a, torch.Generator().manual_seed(2), 2)
    path = str(tmp_path / "out" / "point_cloud.ply")
    a.save_ply(path)
    b = GaussianModel(3)
    b.load_ply(path)
    assert b.optimizer is None
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_refl_strength"):
        assert _bits(getattr(a, name).contiguous()) == _bits(getattr(b, name).contiguous()) and getattr(a, name).shape == getattr(b, name).shape, name
    for key in ("Cubemap_texture", "Cubemap_failv"):
        assert _bits(a.get_envmap.params[key]) == _bits(b.get_envmap.params[key]), key
    bg = torch.zeros(3, device="cuda")
    pipe = types.SimpleNamespace(depth_ratio=0.0, compute_cov3D_python=False)
    with torch.no_grad():
        ra, rb = render_fast(View, a, pipe, bg), render_fast(View, b, pipe, bg)
    assert float(ra["render"].abs().max()) > 0
    for k in ra:
        assert _bits(ra[k]) == _bits(rb[k]), k


# ------------------------------------------------------------------------------------------------- 7. edges
@pytest.mark.parametrize("P", [0, 1])
def test_models_of_no_and_of_one_point(tmp_path, P):
    from scene import GaussianModel
    from scene.ply_io import save_ply
    rs = np.random.RandomState(P)
    path = str(tmp_path / "tiny.ply")
    save_ply(path, rs.randn(P, 3), rs.randn(P, 16, 3), rs.randn(P, 1), rs.randn(P, 1), rs.randn(P, 2) - 3, rs.randn(P, 4),
             cubemap=rs.randn(6, 3, 2, 2), fail_value=rs.randn(3))
    m = GaussianModel(3)
    m.load_ply(path)
    assert m.optimizer is None and m.get_xyz.shape == (P, 3) and m.get_opacity.shape == (P, 1) and m.max_radii2D.shape == (P,)
    with pytest.raises(RuntimeError, match="training_setup"):
        m.densify_and_prune(0.0002, 0.05, torch.zeros(3), 3.0, None)
    with pytest.raises(RuntimeError, match="training_setup"):
        m.capture()
    m.training_setup(_opt())
    assert m.optimizer is not None and m.xyz_gradient_accum.shape == (P, 1)
    env_before = m.get_envmap.params["Cubemap_texture"].detach().clone()
    grads = _synthetic_steps(m, torch.Generator().manual_seed(3), 1)
    assert m._state.optimizer.step_count == 1 and bool((m.get_envmap.params["Cubemap_texture"] != env_before).any())
    viewspace = torch.zeros(P, 3, device="cuda", requires_grad=True)
    viewspace.grad = torch.full((P, 3), 2e-4, device="cuda")
    m.add_densification_stats(viewspace, torch.ones(P, dtype=torch.bool, device="cuda"), torch.full((P,), 0.5, device="cuda"))
    m.add_densification_stats(viewspace, None, torch.full((P,), 0.5, device="cuda"), radii=torch.full((P,), 3, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(m.denom, torch.full((P, 1), 2.0, device="cuda")) and torch.equal(m.max_radii2D, torch.full((P,), 3.0, device="cuda"))
    assert bool(torch.isfinite(m._state.params.flat).all())
    out = str(tmp_path / "tiny_out.ply")
    m.save_ply(out)
    again = GaussianModel(3)
    again.load_ply(out)
    assert _bits(again._state.params.flat) == _bits(m._state.params.flat)
    with pytest.raises(NotImplementedError, match="shard"):
        m.training_setup(_opt(), group=object())
