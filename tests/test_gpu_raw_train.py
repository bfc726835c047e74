"""gsr_train.RawTrainState end to end on the GPU, on the scene of tests/test_gpu_train.py::test_train_state_step_end_to_end (P = 5000,
160 x 120, L = 16): the raw gradients of one step against plain autograd through torch's activations, a 40-step loop with one
densification, the three resets against the reference's expressions, and from_activated.

Bounds are those of tests/test_gpu_raw_step.py: 4 x the error of torch's float32 chain against the float64 restatement
(tests/raw_step_ref.py) plus 2 ulp of the largest value compared.  The rasterizer's backward sums with float atomics, so two backward
passes over the same inputs differ in their last bits; where two passes are compared, 4 x the spread the autograd side shows between two
runs of its own is added, measured in the test."""
import numpy as np
import pytest
import torch

import raw_step_ref as R
from poison import u32

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
P, W, H, L = 5000, 160, 120, 16
NAMES = ["means3D", "shs", "opacities", "scales", "rotations", "refl_strengths"]
ZERO_LRS = dict(position_lr_init=0.0, position_lr_final=0.0, feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0, rotation_lr=0.0, refl_lr=0.0,
                envmap_cubemap_lr=0.0)


def _scene(seed=9, mu=-2.6, P=P):
    import gsr_synth as S
    sc = S.make_scene(P, "S", seed=seed, mu=mu)
    tex, fail = S.make_cubemap(L, 3, seed)
    cam = S.make_camera(W, H)
    act = {k: torch.from_numpy(sc[k]) for k in NAMES}
    act["cubemap"], act["fail"] = torch.from_numpy(tex), torch.from_numpy(fail)
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}
    return sc, act, cam, ct


def _rasterizer(cam, ct):
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    return GaussianRasterizer(GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                                            bg=torch.zeros(3, device="cuda"), scale_modifier=1.0, viewmatrix=ct["viewmatrix"],
                                                            projmatrix=ct["projmatrix"], sh_degree=3, campos=ct["campos"], prefiltered=False, debug=False))


def _image(rast, x, cam, ct, mask):
    """Rasterizer + deferred reflection on the eight tensors x (activated where the rasterizer wants them activated)."""
    from gaussian_renderer import deferred_reflection

    class Env:
        params = {"Cubemap_texture": x["cubemap"], "Cubemap_failv": x["fail"]}
    n = x["means3D"].shape[0]
    means2D = torch.zeros(n, 3, device="cuda", requires_grad=True)
    base, radii, allmap, refl_map, gw = rast(means3D=x["means3D"], means2D=means2D, opacities=x["opacities"], shs=x["shs"], refl_strengths=x["refl_strengths"],
                                             scales=x["scales"], rotations=x["rotations"], env_scope_mask=mask)
    final, _, _ = deferred_reflection(allmap[2:5], base, refl_map, Env, ct["viewmatrix"], (H, W, cam["K"]), ct["R"], ct["T"])
    return final


def _torch_act(name, raw):
    if name in ("opacities", "refl_strengths"):
        return torch.sigmoid(raw)
    if name == "scales":
        return torch.exp(raw)
    if name == "rotations":
        return torch.nn.functional.normalize(raw)
    return raw


def test_raw_gradients_of_one_step_against_autograd_through_torch_activations():
    """Side A: RawTrainState with every learning rate 0, the rasterizer's gradient sink, one optimizer step; the raw gradient is
    exp_avg / (1 - beta1).  Side B: raw leaf tensors -> torch activations -> the same rasterizer and loss under plain autograd -> .grad.
    Yardstick: side B with the activations and the chain rule in float64 (the rasterizer gets the float64 activations rounded once).  The
    activated inputs of the sides differ in their last bit and the rasterizer's gradients answer to that, so the float32 chain's error is
    measured end to end as well.  Bound: 4 x (side B's float32 .grad against the yardstick) + 2 ulp of the group's largest + 4 x the spread
    between two runs of side B (atomics).  The four activated inputs are what torch's activations give, bitwise or within
    4 x (torch float32 on the CPU against float64) + 2 ulp."""
    from gsr_train import RawTrainState
    from utils.loss_utils import photometric_loss
    sc, act, cam, ct = _scene()
    mask = torch.from_numpy(sc["env_scope_mask"]).cuda()
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    st = RawTrainState.from_activated(act, "cuda", lrs=ZERO_LRS)
    st.optimizer.activate()          # (from_activated keeps the values it was given as the activated copy; here: act(raw), as after any step)
    raw0 = st.params.flat.clone()
    # the activated inputs
    for k in RawTrainState.ACTIVATED:
        r = st.p[k].detach().cpu()
        kind = R.ACTIVATED[k]
        want = R.activation(kind, r.numpy().reshape(-1))
        e32 = float(np.abs(_torch_act(k, r).double().numpy().reshape(-1) - want).max())
        got = st.a[k].detach().cpu().numpy().reshape(-1).astype(np.float64)
        err = float(np.abs(got - want).max())
        same = u32(st.a[k].detach().cpu().numpy()).tobytes() == u32(_torch_act(k, st.p[k].detach()).cpu().numpy()).tobytes()
        print(f"activated {k:15s} device {err:.3e} torch float32 (CPU) {e32:.3e} bitwise equal to torch on the device: {same}")
        assert same or err <= 4 * e32 + 2 * ULP * float(np.abs(want).max()), k
    # side A
    rast = _rasterizer(cam, ct)
    sink = st.grads.sink()
    rast.set_grad_sink(sink)
    st.grads.zero_except_(sink)
    photometric_loss(_image(rast, st.render_inputs(), cam, ct, mask), gt, 0.2).backward()
    st.update_learning_rate(1)
    st.set_lr("means3D", 0.0)
    st.optimizer.step()
    torch.cuda.synchronize()
    assert u32(st.params.flat.cpu().numpy()).tobytes() == u32(raw0.cpu().numpy()).tobytes()
    got = st.optimizer.exp_avg.cpu().numpy().astype(np.float64) / (1.0 - R.f32(0.9))

    # side B in float32, twice (the spread of the atomics), and the yardstick
    def side_b():
        leaves = {k: st.p[k].detach().clone().requires_grad_(True) for k in st.params.names}
        x = {k: _torch_act(k, v) for k, v in leaves.items()}
        photometric_loss(_image(_rasterizer(cam, ct), x, cam, ct, mask), gt, 0.2).backward()
        return {k: v.grad.detach().cpu().numpy().reshape(-1).astype(np.float64) for k, v in leaves.items()}

    def yardstick():
        """The same chain with the activations and the chain rule in float64: the rasterizer takes float32, so it is handed the float64
        activations rounded once, and its dL/d(activated) goes through raw_step_ref.raw_gradient."""
        x = {k: _torch_act(k, st.p[k].detach().double()).float().requires_grad_(True) for k in st.params.names}
        photometric_loss(_image(_rasterizer(cam, ct), x, cam, ct, mask), gt, 0.2).backward()
        out = {}
        for k in st.params.names:
            a, b = st.params.slices[k]
            d = x[k].grad.detach().cpu().numpy().reshape(-1).astype(np.float64)
            kind = R.ACTIVATED.get(k, R.NONE)
            out[k] = R.raw_gradient(kind, raw0[a:b].cpu().numpy().astype(np.float64), d) if kind else d
        return out
    g1, g2, g64 = side_b(), side_b(), yardstick()
    for k in st.params.names:
        a, b = st.params.slices[k]
        ref = g64[k]
        scale = float(np.abs(ref).max())
        e32 = float(np.abs(g1[k] - ref).max())
        spread = float(np.abs(g2[k] - g1[k]).max())
        err = float(np.abs(got[a:b] - ref).max())
        bound = 4 * e32 + 2 * ULP * scale + 4 * spread
        print(f"raw gradient {k:15s} device {err:.3e} autograd float32 {e32:.3e} spread of two autograd runs {spread:.3e} bound {bound:.3e} (largest {scale:.3e})")
        if k != "fail":                                # (the fail value only matters for a zero reflection vector)
            assert scale > 0, k
        assert err <= bound, (k, err, bound)


def test_forty_steps_keep_the_rendered_parameters_in_their_domains_and_survive_densification():
    """The loop of tests/test_gpu_train.py::test_training_loop_converges_and_survives_densification on a RawTrainState that starts from the
    perturbed scene.  The loss falls as that test requires; after every step the rendered opacities and reflection strengths lie strictly in
    (0, 1), the scales are positive and every rendered quaternion has norm 1 within 1e-6; the densify_and_prune in the middle returns a
    RawTrainState whose activated buffer is gsr_activate of its raw buffer bit for bit.
    For comparison (printed, not asserted): the same loop on GaussianTrainState, which steps the activated values directly, with a rotation
    learning rate of 0.05 — its quaternion norms leave that band.  Measured on an MI355X: the largest | |q| - 1 | among the rendered
    quaternions over the 40 steps is 1.6e-7 for RawTrainState and 2.2 to 2.5 for GaussianTrainState (two runs; DESIGN.md, "Raw-parameter step")."""
    import gsr_synth as S
    from gaussian_renderer import render
    from gsr_densify import DensifyStats, densify_and_prune
    from gsr_train import GaussianTrainState, RawTrainState
    from utils.loss_utils import photometric_loss
    P0 = 6000
    sc = S.make_scene(P0, "S", seed=13, mu=-2.7)
    tex, fail = S.make_cubemap(L, 3, 13)
    cam = S.make_camera(W, H)
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}

    class View:
        FoVx, FoVy = 2 * np.arctan(cam["tanfovx"]), 2 * np.arctan(cam["tanfovy"])
        image_width, image_height = W, H
        world_view_transform, full_proj_transform, camera_center = ct["viewmatrix"], ct["projmatrix"], ct["campos"]
        HWK, R, T = (H, W, cam["K"]), ct["R"], ct["T"]
        znear, zfar = 0.01, 100.0

    class Pipe:
        depth_ratio, compute_cov3D_python = 0.0, False

    truth = {k: torch.from_numpy(sc[k]) for k in NAMES}
    truth["cubemap"], truth["fail"] = torch.from_numpy(tex), torch.from_numpy(fail)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        gt = render(View, RawTrainState.from_activated(truth, "cuda").model(3), Pipe, bg)["render"].detach().clone()
    g = torch.Generator(device="cpu").manual_seed(1)
    start = {k: v.clone() for k, v in truth.items()}
    start["shs"] = start["shs"] + 0.3 * torch.randn(start["shs"].shape, generator=g)
    start["opacities"] = start["opacities"] * 0.7

    def loop(st, model_of, raw):
        stats = DensifyStats(P0, "cuda")
        losses, worst = [], 0.0
        for it in range(1, 41):
            st.update_learning_rate(it)
            st.grads.zero_()
            pkg = render(View, model_of(st), Pipe, bg)
            loss = photometric_loss(pkg["render"], gt, 0.2)
            normal_error = (1 - (pkg["rend_normal"] * pkg["surf_normal"]).sum(dim=0))[None]      # train.py:182-189
            loss = loss + 0.05 * normal_error.mean()
            loss.backward()
            losses.append(float(photometric_loss(pkg["render"].detach(), gt, 0.2)))
            stats.update(pkg["viewspace_points"].grad, pkg["radii"], pkg["gaussian_weights"])
            st.optimizer.step()
            if it == 20:
                st, stats, info = densify_and_prune(st, stats, 0.0002, 0.05, torch.zeros(3), 5.0, None)
                assert info["after"] == st.p["means3D"].shape[0] and info["after"] > 0
                if raw:
                    assert type(st) is RawTrainState
                    have = st.optimizer.act.clone()
                    st.optimizer.act.fill_(float("nan"))
                    st.optimizer.activate()
                    torch.cuda.synchronize()
                    assert u32(have.cpu().numpy()).tobytes() == u32(st.optimizer.act.cpu().numpy()).tobytes()
            x = st.render_inputs() if raw else st.p
            norms = x["rotations"].detach().double().norm(dim=1)
            worst = max(worst, float((norms - 1).abs().max()))
            if raw:
                for k in ("opacities", "refl_strengths"):
                    v = x[k].detach()
                    assert bool(((v > 0) & (v < 1)).all()), (k, it, float(v.min()), float(v.max()))
                assert bool((x["scales"].detach() > 0).all()), it
                assert float((norms - 1).abs().max()) <= 1e-6, (it, float((norms - 1).abs().max()))
        return losses, worst

    losses, worst = loop(RawTrainState.from_activated(start, "cuda", spatial_lr_scale=1.0), lambda st: st.model(3), True)
    print("RawTrainState: losses", [round(x, 5) for x in losses[:3]], [round(x, 5) for x in losses[16:23]], [round(x, 5) for x in losses[-3:]],
          "largest | |q| - 1 | rendered: %.3e" % worst)
    assert np.isfinite(losses).all()
    assert np.mean(losses[16:20]) < 0.8 * np.mean(losses[:3]), (losses[:3], losses[16:20])
    assert np.mean(losses[-3:]) < np.mean(losses[20:23]), (losses[20:23], losses[-3:])

    def activated_model(st):
        class Env:
            params = {"Cubemap_texture": st.p["cubemap"], "Cubemap_failv": st.p["fail"]}

        class PC:
            get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (st.p["means3D"], st.p["opacities"], st.p["scales"],
                                                                                       st.p["rotations"], st.p["shs"], st.p["refl_strengths"])
            active_sh_degree, get_envmap = 3, Env
        return PC
    _, worst_act = loop(GaussianTrainState(start, "cuda", spatial_lr_scale=1.0, lrs=dict(rotation_lr=0.05)), activated_model, False)
    print("GaussianTrainState with rotation_lr = 0.05: largest | |q| - 1 | rendered: %.3e" % worst_act)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "exclusive_msk"])
def test_resets_follow_the_reference_and_refresh_the_activated_copy(masked):
    """reset_opacity, reset_refl, reset_scale (scene/gaussian_model.py:264-294) against the reference's expressions restated in torch on the
    raw views; both moments of the group are zero afterwards, every other group keeps its bits (raw and moments), the activated copy is
    gsr_activate of the new raw values."""
    from gsr_train import RawTrainState, inverse_sigmoid
    sc, act, cam, ct = _scene(P=1031)
    msk = (torch.arange(1031) % 3 == 0).cuda() if masked else None

    def fresh():
        st = RawTrainState.from_activated(act, "cuda")
        with torch.no_grad():
            st.p["refl_strengths"][::7] = -9.0          # below init_refl_value = 1e-3 (logit -6.9): reset_refl lifts these
        st.optimizer.activate()
        st.optimizer.exp_avg.fill_(0.25)
        st.optimizer.exp_avg_sq.fill_(0.5)
        return st

    def want_opacity(raw):
        new = inverse_sigmoid(torch.min(torch.sigmoid(raw), torch.ones_like(raw) * 0.01))
        return new

    def want_refl(raw):
        return inverse_sigmoid(torch.max(torch.sigmoid(raw), torch.ones_like(raw) * 1e-3))

    def want_scale(raw):
        scales = torch.exp(raw)
        rmin_axis = (torch.ones_like(scales) * 1.5).scatter(1, torch.argmin(scales, dim=-1, keepdim=True), 1)
        return torch.log(scales * rmin_axis)

    for group, call, want in (("opacities", lambda st: st.reset_opacity(0.01, exclusive_msk=msk), want_opacity),
                              ("refl_strengths", lambda st: st.reset_refl(1e-3, exclusive_msk=msk), want_refl),
                              ("scales", lambda st: st.reset_scale(1.5, exclusive_msk=msk), want_scale)):
        st = fresh()
        before = {k: x.clone() for k, x in (("raw", st.params.flat), ("m", st.optimizer.exp_avg), ("v", st.optimizer.exp_avg_sq))}
        raw = st.p[group].detach().clone()
        new = want(raw)
        if masked:
            new[msk] = raw[msk]
        call(st)
        torch.cuda.synchronize()
        assert torch.equal(st.p[group].detach(), new), group
        assert bool((st.p[group].detach() != raw).any()), group
        if masked:
            assert torch.equal(st.p[group].detach()[msk], raw[msk]), group
        names = st.params.names
        for i, k in enumerate(names):
            a = st.params.slices[k][0]
            end = st.params.slices[names[i + 1]][0] if i + 1 < len(names) else st.params.total
            if k == group:
                assert not st.optimizer.exp_avg[a:end].any() and not st.optimizer.exp_avg_sq[a:end].any(), k
            else:
                for q, t in (("raw", st.params.flat), ("m", st.optimizer.exp_avg), ("v", st.optimizer.exp_avg_sq)):
                    assert torch.equal(t[a:end], before[q][a:end]), (group, k, q)
        have = st.optimizer.act.clone()
        st.optimizer.act.fill_(float("nan"))
        st.optimizer.activate()
        torch.cuda.synchronize()
        assert u32(have.cpu().numpy()).tobytes() == u32(st.optimizer.act.cpu().numpy()).tobytes(), group
        r64 = st.p[group].detach().cpu().numpy().reshape(-1)
        ref = R.activation(R.ACTIVATED[group], r64)
        got = st.a[group].detach().cpu().numpy().reshape(-1).astype(np.float64)
        e32 = float(np.abs(_torch_act(group, st.p[group].detach().cpu()).double().numpy().reshape(-1) - ref).max())
        assert np.abs(got - ref).max() <= 4 * e32 + 2 * ULP * np.abs(ref).max(), group
        if group == "opacities":
            assert float(st.a[group].max()) <= 0.01 * (1 + 1e-5) or masked


def test_from_activated_renders_what_the_activated_state_renders():
    """RawTrainState.from_activated(init_from_point_cloud(...)) against the same tensors handed to GaussianTrainState: the rendered images,
    bit for bit.  from_activated keeps the values it was given as the activated copy (the round trip through float32 raw values, log then
    exp, inverse_sigmoid then sigmoid, normalize of a unit quaternion, moves most of them by an ulp; it is printed per group)."""
    from gaussian_renderer import render
    from gsr_init import init_from_point_cloud
    from gsr_train import GaussianTrainState, RawTrainState
    sc, act, cam, ct = _scene(P=2000)
    colors = torch.rand(2000, 3, generator=torch.Generator().manual_seed(2))
    gen = torch.Generator(device="cuda").manual_seed(7)
    tensors = init_from_point_cloud(act["means3D"].cuda(), colors, sh_degree=3, cubemap_resolution=L, generator=gen)

    class View:
        FoVx, FoVy = 2 * np.arctan(cam["tanfovx"]), 2 * np.arctan(cam["tanfovy"])
        image_width, image_height = W, H
        world_view_transform, full_proj_transform, camera_center = ct["viewmatrix"], ct["projmatrix"], ct["campos"]
        HWK, R, T = (H, W, cam["K"]), ct["R"], ct["T"]
        znear, zfar = 0.01, 100.0

    class Pipe:
        depth_ratio, compute_cov3D_python = 0.0, False
    raw = RawTrainState.from_activated(tensors, "cuda")
    flat = GaussianTrainState(tensors, "cuda")

    class Env:
        params = {"Cubemap_texture": flat.p["cubemap"], "Cubemap_failv": flat.p["fail"]}

    class PC:
        get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (flat.p["means3D"], flat.p["opacities"], flat.p["scales"],
                                                                                   flat.p["rotations"], flat.p["shs"], flat.p["refl_strengths"])
        active_sh_degree, get_envmap = 3, Env
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        a = render(View, raw.model(3), Pipe, bg)["render"]
        b = render(View, PC, Pipe, bg)["render"]
    print("rendered images: largest difference %.3e, pixels that differ %d" % (float((a - b).abs().max()), int((a != b).sum())))
    assert float(b.abs().max()) > 0
    assert torch.equal(a, b)
    for k in RawTrainState.ACTIVATED:
        assert torch.equal(raw.a[k].detach(), flat.p[k].detach()), k
    # what the first step replaces the copy by: act(raw), the round trip through float32 raw values (printed; an ulp)
    raw.optimizer.activate()
    for k in RawTrainState.ACTIVATED:
        d = (raw.a[k].detach() - flat.p[k].detach()).abs()
        rel = float((d / flat.p[k].detach().abs()).max())
        print(f"round trip {k:15s} largest difference {float(d.max()):.3e} relative {rel:.3e} elements that differ {int((d != 0).sum())} of {d.numel()}")