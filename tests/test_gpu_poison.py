"""No result may depend on what an uninitialised buffer held.

Every output plane, workspace and scratch region of the package comes from `torch.empty` and is zero in a fresh process, but whatever the
caching allocator returns in training.  Each operation below runs under tests/poison.py with every such buffer pre-filled with 0x00 (the
baseline, first), 0xFF (float NaN, int -1) and 0x01 (finite garbage): what is deterministic must be the same bits under all three, every
output element finite (under 0xFF an element nobody wrote is NaN), culled Gaussians exactly zero, and everything summed with float
atomics within the suite's own gates of the oracle under each pattern.  The order of the file is the order of risk: per-pixel passes
first, the rasterizers' binning (whose state a stale byte turns into an index) and the fused path last.

P = 0: the library returns zero planes, the colour included, as the reference does for an empty scene (tests/test_gpu_api_paths.py); the
image equals the background where Gaussians exist and all are culled.  Both are held here at 1x1 and 17x15.

Each test prints `POISON <operation>: <allocations> allocations, <bytes> bytes` per pattern."""
import numpy as np
import pytest
import torch

import loss_bounds as LB
import metrics_ref as MR
import poison
from helpers import GATE_BUDGET, HipGauss, HipSurfel, S, grad_gate, rel_maxnorm, scene_kwargs, to_cuda
from poison import PATTERNS, poisoned

pytestmark = pytest.mark.gpu
U = LB.U


@pytest.fixture(autouse=True)
def _python_allocations():
    """The compiled binding allocates in C++: every call of this file takes the ctypes marshaling, whose allocations are Python's."""
    import _gsr
    with poison.ctypes_binding():
        assert _gsr.PYBIND is None
        yield


def across(what, fn):
    """fn() under each pattern, 0x00 first; the harness must have been live in each.  Returns the three results."""
    out = []
    for pattern in PATTERNS:
        with poisoned(pattern) as ps:
            r = fn()
            torch.cuda.synchronize()
        print("POISON %s [0x%02X]: %d allocations, %d bytes" % (what, pattern, ps.count, ps.bytes))
        assert ps.count > 0, (what, "no poisoned allocation: the harness is not live for this operation")
        out.append(r)
    return out


def npy(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(results, what, keys=None):
    """Every array of the later results is the first's, bit for bit."""
    base = results[0]
    for pattern, r in zip(PATTERNS[1:], results[1:]):
        for k in (keys or base.keys()):
            if base[k] is None:
                assert r[k] is None
                continue
            a, b = np.asarray(base[k]), np.asarray(r[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
            np.testing.assert_array_equal(poison.u32(b), poison.u32(a), err_msg="%s: %s under 0x%02X" % (what, k, pattern))


def all_finite(r, what, keys=None):
    for k in (keys or r.keys()):
        if r[k] is not None and np.asarray(r[k]).dtype.kind == "f":
            assert np.isfinite(r[k]).all(), (what, k, "not finite: an element nobody wrote?")


# =============================================================================================== losses, surface pass
LOSS_SHAPES = [(3, 1, 1), (3, 67, 131), (3, 33, 33)]      # 33 = SSIM_T + 1: one tile more than the 32-pixel tile each way
_loss_refs = {}


def _loss_case(shape):
    if shape not in _loss_refs:
        x, y = LB.loss_pair("uniform", shape, 5 + shape[1])
        n = x.size
        _loss_refs[shape] = (x, y, LB.ssim_reference(x, y, 0.8 / n, -0.2 / n), LB.ssim_reference(x, y, 1.0 / n, 0.0)[0]["grad"])
    return _loss_refs[shape]


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_photometric_ssim_and_l1_losses(shape):
    """Sums reduced in a fixed order (csrc/gsr_loss.hip): values and image gradient the same bits under every pattern, and within the
    float64 bounds of loss_bounds.py.  The scalars are sum / n and a two-term combination in float32: two more roundings each."""
    from utils.loss_utils import clear_cache, l1_loss, photometric_loss, ssim
    x, y, (ref, bnd), _ = _loss_case(shape)
    n = x.size
    X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()

    def run():
        clear_cache()
        a = X.clone().requires_grad_(True)
        loss = photometric_loss(a, Y, 0.2)
        loss.backward()
        clear_cache()
        with torch.no_grad():
            l1, ss = l1_loss(X, Y), ssim(X, Y)
        clear_cache()
        return dict(loss=npy(loss), grad=npy(a.grad), l1=npy(l1), ssim=npy(ss))
    res = across("photometric_loss %s" % (shape,), run)
    same_bits(res, "photometric_loss")
    for r in res:
        all_finite(r, "photometric_loss")
        LB.check(r["grad"], ref["grad"], bnd["grad"], what="grad")
        want_l1, want_ss = ref["l1"] / n, ref["ssim"] / n
        assert abs(float(r["l1"]) - want_l1) <= bnd["l1"] / n + 2 * U * abs(want_l1)
        assert abs(float(r["ssim"]) - want_ss) <= bnd["ssim"] / n + 2 * U * abs(want_ss)
        want = 0.8 * want_l1 + 0.2 * (1.0 - want_ss)
        assert abs(float(r["loss"]) - want) <= 0.8 * bnd["l1"] / n + 0.2 * bnd["ssim"] / n + 8 * U * (abs(want_l1) + 1.0 + abs(want_ss))


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("H,W", [(1, 1), (67, 131), (33, 33)])
def test_normal_consistency_loss(H, W, use_mask):
    """One fixed-order sum: the same bits under every pattern; against the reference's expression in float64.  Value: a pixel's term
    1 - rn . sn passes three products and three sums of magnitudes <= 2 (8 U), the block reduction loss_bounds.NSUM more additions of
    the partial sums, the scale by lambda / n two roundings.  Gradients: to 1e-6 of their maximum, as test_gpu_train.py holds them."""
    from utils.loss_utils import normal_consistency_loss
    g = torch.Generator().manual_seed(H * 1000 + W)
    rn0 = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0).cuda()
    sn0 = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0).cuda()
    mask = (torch.rand(1, H, W, generator=g) < 0.7).float().cuda() if use_mask else None
    lam = 0.05
    rd, sd = rn0.double().requires_grad_(True), sn0.double().requires_grad_(True)
    err = (1 - (rd * sd).sum(dim=0))[None]
    if use_mask:
        err = err * mask.double()
    ref = lam * err.mean()
    (ref * 3.0).backward()
    bound = lam * (8 * U + (LB.NSUM + 2) * U * float(err.detach().abs().mean())) + 4 * U * abs(float(ref))

    def run():
        rn, sn = rn0.clone().requires_grad_(True), sn0.clone().requires_grad_(True)
        loss = normal_consistency_loss(rn, sn, lam, mask)
        (loss * 3.0).backward()
        return dict(loss=npy(loss), g_rn=npy(rn.grad), g_sn=npy(sn.grad))
    res = across("normal_consistency_loss %dx%d mask=%s" % (H, W, use_mask), run)
    same_bits(res, "normal_consistency_loss")
    for r in res:
        all_finite(r, "normal_consistency_loss")
        assert abs(float(r["loss"]) - float(ref)) <= bound, (float(r["loss"]), float(ref), bound)
        for a, b in ((r["g_rn"], rd.grad), (r["g_sn"], sd.grad)):
            b = b.cpu().numpy()
            assert np.abs(a - b).max() <= 1e-6 * max(float(np.abs(b).max()), 1e-30)


@pytest.mark.parametrize("ratio", [0.0, 0.3])
@pytest.mark.parametrize("H,W", [(1, 1), (67, 131), (33, 33)])
def test_surface_pass_depth_to_normal(H, W, ratio):
    """gaussian_renderer._SurfacePass (gsr_surface_forward / _backward): gathers, no atomics — the same bits under every pattern, and
    within the float64 bounds of loss_bounds.surface_reference."""
    import gaussian_renderer as gr
    am, ray = LB.surface_scene(H, W, 3 + H)
    rs = np.random.RandomState(H + W)
    gsd, gsn = rs.randn(H, W).astype(np.float32), rs.randn(3, H, W).astype(np.float32)
    ref, bnd, skip = LB.surface_reference(am, ray, ratio, gsd, gsn)
    A0, R, GD, GN = (torch.from_numpy(a).cuda() for a in (am, ray, gsd, gsn))

    def run():
        A = A0.clone().requires_grad_(True)
        sd, sn = gr._SurfacePass.apply(A, R, ratio)
        ((sd[0] * GD).sum() + (sn * GN).sum()).backward()
        return dict(sd=npy(sd)[0], sn=npy(sn), g=npy(A.grad))
    res = across("surface_pass %dx%d ratio=%g" % (H, W, ratio), run)
    same_bits(res, "surface_pass")
    for r in res:
        for k in ("sd", "sn", "g"):
            LB.check(r[k], ref[k], bnd[k], skip[k], "surface_pass " + k)
        assert (r["g"][[2, 3, 4, 6, 7]] == 0).all()


# =============================================================================================== metrics, viewer
@pytest.mark.parametrize("variant", MR.VARIANTS)
def test_metrics_table_rows_and_8bit_images(variant):
    """MetricsTable.image: its scratch is poisoned, its rows are the caller's table.  Rows and 8-bit images the same bits under every
    pattern, the sums within the float64 bounds of metrics_ref.py, the images torch's float32 chain level for level; rows never written
    keep their NaN."""
    from gsr_eval import MetricsTable
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cases = []
    for i, shape in enumerate(((3, 1, 1), (3, 33, 31), (3, 43, 75))):
        v, g = MR.image_pair("uniform", shape, 10 + i)
        kw = MR.presentation_inputs(variant, shape, 10 + i)
        pv, pg, _, _ = MR.present(v, g, **kw)
        cases.append((v, g, kw, MR.image_sums_reference(pv, pg), MR.torch_present(v, g, **kw)[2:] if kw.get("quantize") else None,
                      [dev(v), dev(g), dev(kw.get("alpha")), dev(kw.get("gt_mask")), dev(kw.get("background"))]))

    def run():
        out = {}
        table = MetricsTable(len(cases) + 1, "cuda")
        for i, (v, g, kw, _, _, (dv, dg, da, dm, db)) in enumerate(cases):
            q = bool(kw.get("quantize"))
            u8 = (torch.empty(v.shape, dtype=torch.uint8, device="cuda"), torch.empty(v.shape, dtype=torch.uint8, device="cuda")) if q else (None, None)
            table.image(i, dv, dg, clamp=kw.get("clamp", False), alpha=da, gt_mask=dm, background=db, quantize8=q, img_u8=u8[0], gt_u8=u8[1])
            out["img%d" % i], out["gt%d" % i] = npy(u8[0]), npy(u8[1])
        out["rows"] = table.result()
        return out
    res = across("MetricsTable.image " + variant, run)
    same_bits(res, "MetricsTable.image")
    for r in res:
        assert np.isnan(r["rows"][len(cases)]).all()
        for i, (v, g, kw, (ref, bnd), levels, _) in enumerate(cases):
            for j, k in enumerate(("sse", "sad", "ssim")):
                MR.check_scalar(r["rows"][i, j], ref[k], bnd[k], "%s row %d %s" % (variant, i, k))
            assert r["rows"][i, 3] == v.size
            if levels is not None:
                np.testing.assert_array_equal(r["img%d" % i], levels[0])
                np.testing.assert_array_equal(r["gt%d" % i], levels[1])


@pytest.mark.parametrize("family", ["random", "degenerate"])
def test_normal_mae(family):
    """utils.mae_utils.angular_error_map / compute_mae: the map (NaN exactly where the reference has it) and the mean the same bits under
    every pattern, within the bounds of metrics_ref.py."""
    from utils.mae_utils import angular_error_map, compute_mae
    for i, (H, W) in enumerate(MR.MAE_SHAPES):
        p, g = MR.normal_pair(family, H, W, 50 + i)
        ang, bound, ambiguous = MR.angular_error_reference(p, g)
        assert not ambiguous.any()
        s, valid, invalid, b = MR.angle_sum_reference(ang, bound)
        P_, G_ = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
        res = across("normal_mae %s %dx%d" % (family, H, W), lambda: dict(map=npy(angular_error_map(P_, G_)), mae=npy(compute_mae(P_[None], G_[None]))))
        same_bits(res, "normal_mae")
        for r in res:
            LB.check(r["map"], ang, bound, what="angle map")
            if invalid:
                assert np.isnan(r["mae"])
            else:
                assert abs(float(r["mae"]) - s / valid) <= b / valid + 2 * MR.U * s / valid


@pytest.mark.parametrize("masks", [False, True])
def test_evaluate_views(masks):
    """evaluate_views (render_fast under no_grad -> gsr_image_metrics / gsr_normal_mae per view, 8-bit images kept): every number and
    every image the same bits under every pattern; the images are torch's presentation of the render, the sums within their bounds."""
    from gaussian_renderer import render_fast
    from gsr_eval import evaluate_views
    from test_gpu_dropin import _Pipe, _model, _scene, _view
    W, H = 64, 48
    t, env = _scene(3000, 5, -1.0, 16)
    PC = _model(t, env)
    bg = torch.tensor([0.1, 0.95, 0.3], device="cuda")
    rs = np.random.RandomState(8)
    views, normals = [], []
    for i, eye in enumerate(((0.4, -0.3, -1.0), (-0.5, 0.2, -1.2))):
        View = _view(S.look_at_camera(W, H, eye=eye, target=(0, 0, 5)), W, H)
        View.original_image = torch.from_numpy(rs.rand(3, H, W).astype(np.float32)).cuda()
        View.gt_alpha_mask = torch.from_numpy((rs.rand(1, H, W) < 0.8).astype(np.float32)).cuda() if masks else None
        views.append(View)
        normals.append(torch.from_numpy(MR.normal_pair("random", H, W, 60 + i)[1]).cuda())

    def run():
        out = evaluate_views(views, PC, _Pipe, bg, gt_normals=normals, keep_images=True)
        r = {k: np.asarray(out["per_view"][k], np.float64) for k in ("PSNR", "SSIM", "MAE")}
        for i, (a, b) in enumerate(out["images"]):
            r["img%d" % i], r["gt%d" % i] = npy(a), npy(b)
        return r
    res = across("evaluate_views masks=%s" % masks, run)
    same_bits(res, "evaluate_views")
    for i, View in enumerate(views):
        with torch.no_grad():
            pkg = render_fast(View, PC, _Pipe, bg)
        kw = dict(clamp=True, quantize=True)
        if masks:
            kw.update(alpha=npy(pkg["rend_alpha"])[0], gt_mask=npy(View.gt_alpha_mask)[0], background=npy(bg))
        v, g = npy(pkg["render"]), npy(View.original_image)
        pv, pg, _, _ = MR.present(v, g, **kw)
        _, _, tlv, tlg = MR.torch_present(v, g, **kw)
        ref, bnd = MR.image_sums_reference(pv, pg)
        for r in res:
            np.testing.assert_array_equal(r["img%d" % i], tlv)
            np.testing.assert_array_equal(r["gt%d" % i], tlg)
            assert abs(r["PSNR"][i] - MR.psnr(ref["sse"], v.size)) <= MR.psnr_bound(ref["sse"], bnd["sse"])
            assert abs(r["SSIM"][i] - ref["ssim"] / v.size) <= bnd["ssim"] / v.size


@pytest.mark.parametrize("family,mode", [("smooth", "RGB"), ("normals", "Normal"), ("smooth", "Depth"), ("constant", "Alpha"), ("normals", "Curvature"),
                                         ("constant", "Curvature")])
def test_viewer_present_bytes(family, mode):
    """present_bytes / render_net_image: the min/max slots of a colour-mapped mode live in scratch that utils.image_utils caches per
    stream, so the cache is dropped inside each pattern.  Frames and float images the same bits under every pattern, and what
    tests/viewer_ref.py says they are (test_gpu_viewer.check_mode: bit for bit where the order of operations is fixed, the curvature's
    gradient within its bound).  'constant': max == min."""
    import test_gpu_viewer as TV
    import viewer_ref as VR
    from utils import image_utils as IU
    m = VR.ITEMS.index(mode)
    shapes = [(H, W) for H, W in ((1, 1), (33, 31), (64, 65)) if VR.defined(family, VR.ITEMS, m, H, W)]
    assert shapes, "no shape at which this family and mode are defined: nothing would be checked"
    for H, W in shapes:
        _, _, drgb, dpkg, _ = TV._case(family, H, W)

        def run():
            IU._scratch.clear()
            TV.check_mode(family, H, W, m)
            IU._scratch.clear()
            r = dict(frame=npy(IU.present_bytes(drgb, dpkg, VR.ITEMS, m)), image=npy(IU.render_net_image(drgb, dpkg, VR.ITEMS, m, None)))
            IU._scratch.clear()
            return r
        res = across("present_bytes %s %s %dx%d" % (family, mode, H, W), run)
        same_bits(res, "present_bytes")
        for r in res:
            all_finite(r, "present_bytes")


# =============================================================================================== densification, KNN
def test_densify_stats_and_densify_and_prune():
    """DensifyStats.update over two views, then densify_and_prune with supplied noise at P = 9001: statistics, surviving rows and both
    Adam moments the same bits under every pattern (pure data movement and elementwise arithmetic), the new statistics all zero."""
    from gsr_densify import densify_and_prune
    from test_gpu_densify import _setup
    P = 9001
    sc, st, _, names = _setup(P, 11, -3.2)
    rs = np.random.RandomState(5)
    ups = [(torch.from_numpy((rs.randn(P, 3) * 1e-3).astype(np.float32)).cuda(),
            torch.from_numpy((rs.rand(P) < 0.6).astype(np.int32) * rs.randint(1, 40, P).astype(np.int32)).cuda(),
            torch.from_numpy((rs.rand(P) * (rs.rand(P) < 0.5)).astype(np.float32)).cuda()) for _ in range(2)]
    denom = rs.randint(0, 5, P).astype(np.float32)
    dw = rs.randint(0, 4, P).astype(np.float32)
    vals = dict(xyz_gradient_accum=(rs.rand(P) * 8e-4 * denom).astype(np.float32), denom=denom, denom_w=dw, accum_w=(rs.rand(P) * 0.05 * dw).astype(np.float32),
                max_radii2D=rs.randint(0, 60, P).astype(np.float32))
    vals = {k: torch.from_numpy(v).cuda() for k, v in vals.items()}
    with torch.no_grad():
        st.p["scales"].copy_(torch.from_numpy(np.log(np.exp(rs.randn(P, 2) * 1.2) * 0.03).astype(np.float32)))
    noise = torch.from_numpy(rs.randn(2 * P, 2).astype(np.float32)).cuda()
    from gsr_densify import DensifyStats
    k = densify_and_prune(st, _filled(DensifyStats(P, "cuda"), vals), 0.0002, 0.05, torch.zeros(3), 3.0, 20)[2]["split"]
    assert k > 20

    def run():
        seen = DensifyStats(P, "cuda")
        for g, radii, w in ups:
            seen.update(g, radii, w)
        new, new_stats, info = densify_and_prune(st, _filled(DensifyStats(P, "cuda"), vals), 0.0002, 0.05, torch.zeros(3), 3.0, 20, noise=noise[:2 * k])
        assert float(new_stats.buf.abs().max()) == 0 and new_stats.buf.shape == (5, new.p["means3D"].shape[0])
        assert info["split"] == k and info["cloned"] > 20
        return dict(seen=npy(seen.buf), params=npy(new.params.flat), m=npy(new.optimizer.exp_avg), v=npy(new.optimizer.exp_avg_sq),
                    counts=np.array([info[c] for c in sorted(info) if isinstance(info[c], int)]))
    res = across("densify_and_prune P=9001", run)
    same_bits(res, "densify_and_prune")
    for r in res:
        all_finite(r, "densify_and_prune")


def _filled(stats, vals):
    for k, v in vals.items():
        getattr(stats, k).copy_(v)
    return stats


@pytest.mark.parametrize("P", [3, 65, 4097])
def test_knn_mean_distance(P):
    """simple_knn.distCUDA2: out and scratch (cell lists, sort temporaries) are poisoned.  The same bits under every pattern; against
    scipy's cKDTree in float64 to 1e-6 relative as tests/test_gpu_knn.py; with three points the missing third neighbour counts as FLT_MAX."""
    from scipy.spatial import cKDTree
    from simple_knn._C import distCUDA2
    pts = np.ascontiguousarray(np.random.RandomState(P).uniform(-1.0, 1.0, (P, 3)), dtype=np.float32)
    x = pts.astype(np.float64)
    d = cKDTree(x).query(x, k=min(4, P))[0][:, 1:] ** 2
    if P < 4:
        d = np.concatenate([d, np.full((P, 4 - P), float(np.finfo(np.float32).max))], axis=1)
    want = d.mean(axis=1)
    X = torch.from_numpy(pts).cuda()
    res = across("distCUDA2 P=%d" % P, lambda: dict(d=npy(distCUDA2(X))))
    same_bits(res, "distCUDA2")
    for r in res:
        assert np.isfinite(r["d"]).all()
        assert (np.abs(r["d"].astype(np.float64) - want) / want).max() <= 1e-6


# =============================================================================================== cubemap lookup
@pytest.mark.parametrize("interp,seamless", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("B", [1, 255, 257])
def test_cubemap_encoder(B, interp, seamless):
    """cubemapencoder.cubemap_encode: features and direction gradients (one thread each) the same bits under every pattern; the texture
    and fail-value gradients are float-atomic sums, held to the oracle under each pattern with tests/test_gpu_cubemap.py's tolerances."""
    from cubemapencoder.cubemap_encoder import cubemap_encode
    from oracle import oracle as orc
    L, C = 16, 3
    g = torch.Generator().manual_seed(B)
    d = torch.randn(B, 3, generator=g)
    special = torch.tensor([[0, 0, 0], [1, 1, 1], [1, -1, 0], [1, 0.999, 0.2], [1, 1 - 1.0 / L, 1 - 1.0 / L], [0, 0, -1]], dtype=torch.float32)
    n = min(B, len(special))
    d[B - n:] = special[:n]                      # B = 1: the zero vector alone (the fail value)
    cm, fv, go = torch.rand(6, C, L, L, generator=g) - 0.5, torch.randn(C, generator=g), torch.randn(C, B, generator=g)
    ref = orc.cubemap_forward(d.numpy(), cm.numpy(), fv.numpy(), interp, seamless)
    rin, rcm, rf = orc.cubemap_backward(go.numpy(), d.numpy(), cm.numpy(), interp, seamless)
    D0, CM0, FV0, GO = d.cuda(), cm.cuda(), fv.cuda(), go.cuda()

    def run():
        D, CM, FV = (t.clone().requires_grad_(True) for t in (D0, CM0, FV0))
        out = cubemap_encode(D, CM, FV, interp, seamless)
        (out * GO).sum().backward()
        return dict(out=npy(out), g_dirs=npy(D.grad), g_tex=npy(CM.grad), g_fail=npy(FV.grad))
    res = across("cubemap_encode B=%d interp=%d seamless=%d" % (B, interp, seamless), run)
    same_bits(res, "cubemap_encode", keys=("out", "g_dirs"))
    for r in res:
        all_finite(r, "cubemap_encode")
        np.testing.assert_allclose(r["out"], ref, rtol=1e-5, atol=2e-6)
        assert rel_maxnorm(r["g_tex"], rcm) <= 1e-5 and rel_maxnorm(r["g_fail"], rf) <= 1e-5 and rel_maxnorm(r["g_dirs"], rin) <= 1e-4


# =============================================================================================== rasterizers
FORWARD_S = ("color", "radii", "allmap", "refl_strength_map", "gaussian_weights")
FORWARD_G = ("color", "radii", "invdepth", "normal_map", "refl_strength_map")
STATE = ("tiles_touched", "point_offsets", "keys", "point_list", "ranges", "n_contrib", "final_T")
GRADS_S = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_drefl_strengths", "dL_dscales", "dL_drotations")
GRADS_G = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dnormals", "dL_drefl_strengths", "dL_dscales", "dL_drotations")
_raster_refs = {}


def _dead_scene(variant, P, W, H, seed, mu, dead):
    """The scene, the float32 oracle's forward and gradients (computed once per scene, never modified) and the device inputs.  `dead`:
    a range of Gaussians moved behind the camera — 64..127 is one whole wave of the preprocess kernel, which then returns without storing
    its records; 0..255 one whole workgroup."""
    key = (variant, P, W, H, seed, dead)
    if key not in _raster_refs:
        from oracle import oracle as orc
        kw, _, _ = scene_kwargs(variant, P, W, H, seed, mu, 3, (0.2, 0.1, 0.3))
        kw["means3D"] = kw["means3D"].copy()
        kw["means3D"][dead[0]:dead[1], 2] = -np.abs(kw["means3D"][dead[0]:dead[1], 2]) - 1.0
        g = S.make_upstream_grads(H, W, seed)
        _raster_refs[key] = [kw, g, None, to_cuda(kw), {k: torch.from_numpy(v).cuda() for k, v in g.items()}, orc]
    return _raster_refs[key]


def _oracle_of(case, variant, antialiasing=False):
    if case[2] is None or case[2][0] != antialiasing:
        kw, g, orc = case[0], case[1], case[5]
        if variant == "S":
            o = orc.SurfelOracle(np.float32)
            ref = o.forward(**kw)
            gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dallmap=g["dL_dplanes"], dL_drefl_strength_map=g["dL_drefl"])
        else:
            o = orc.GaussOracle(np.float32)
            ref = o.forward(antialiasing=antialiasing, **kw)
            gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dinvdepth=g["dL_dinvdepth"], dL_dnormal_map=g["dL_dnormal"], dL_drefl_strength_map=g["dL_drefl"])
        case[2] = (antialiasing, ref, gr, o.state("radii") > 0)
    return case[2][1:]


def _raster_run(variant, kwc, gc, antialiasing=False):
    """Forward + backward on device inputs; outputs, fetched state and gradients as numpy."""
    if variant == "S":
        hip = HipSurfel(kwc)
        loss = (hip.color * gc["dL_dcolor"]).sum() + (hip.allmap * gc["dL_dplanes"]).sum() + (hip.refl_map * gc["dL_drefl"]).sum()
        leaves = dict(dL_dmeans3D=hip.means3D, dL_dmeans2D=hip.means2D, dL_dopacity=hip.opac, dL_dsh=hip.shs, dL_drefl_strengths=hip.refl,
                      dL_dscales=hip.scales, dL_drotations=hip.rots)
    else:
        hip = HipGauss(kwc, antialiasing=antialiasing)
        loss = ((hip.color * gc["dL_dcolor"]).sum() + (hip.invdepth * gc["dL_dinvdepth"]).sum() + (hip.normal_map * gc["dL_dnormal"]).sum()
                + (hip.refl_map * gc["dL_drefl"]).sum())
        leaves = dict(dL_dmeans3D=hip.means3D, dL_dmeans2D=hip.means2D, dL_dopacity=hip.opac, dL_dsh=hip.shs, dL_dnormals=hip.normals,
                      dL_drefl_strengths=hip.refl, dL_dscales=hip.scales, dL_drotations=hip.rots)
    r = {k: v for k, v in hip.out().items() if isinstance(v, np.ndarray)}
    r["num_rendered"] = np.array([hip.R])
    vis = r["radii"] > 0
    for name in STATE:
        r[name] = hip.state(name)
    r["depths_visible"] = hip.state("depths")[vis]
    r["clamped_visible"] = hip.state("clamped")[vis]
    loss.backward()
    for k, leaf in leaves.items():
        r[k] = npy(leaf.grad)
    return r


def _check_raster(variant, res, ref, gr, what):
    fwd, grads = (FORWARD_S, GRADS_S) if variant == "S" else (FORWARD_G, GRADS_G)
    same_bits(res, what, keys=fwd + STATE + ("num_rendered", "depths_visible", "clamped_visible"))
    for r in res:
        all_finite(r, what, keys=fwd + grads + ("final_T",))
        assert int(r["num_rendered"][0]) == ref["num_rendered"]
        np.testing.assert_array_equal(r["radii"], ref["radii"])
        culled = r["radii"] == 0
        assert culled.sum() >= 64
        if variant == "S":
            assert (r["gaussian_weights"][culled] == 0).all()
        for k in grads:
            a, b = r[k].reshape(gr[k].shape), gr[k]
            assert (a[culled] == 0).all(), (what, k, "a culled Gaussian has a gradient")
            if np.abs(b).max() == 0:
                assert np.abs(a).max() == 0, k
                continue
            assert rel_maxnorm(a, b) <= 1e-4, (what, k, rel_maxnorm(a, b))
            assert grad_gate(a, b, 1e-4, 1e-5) <= max(GATE_BUDGET, 2.0 / a.size), (what, k, "elementwise gate")


def _with_options(options, fn):
    import _gsr
    try:
        for k, v in options.items():
            _gsr.set_option(k, v)
        return fn()
    finally:
        _gsr.set_option("sort_driver", 1)
        _gsr.set_option("emit_items", 0)


SURFEL_SCENES = {"P257": (257, 96, 64, 61, -1.6, (64, 128)), "P4097": (4097, 200, 136, 62, -3.0, (64, 128)),
                 "P4097_dead_workgroup": (4097, 200, 136, 63, -3.0, (0, 256)), "P3001_gathered_grid": (3001, 4112, 48, 64, -3.2, (64, 128))}


@pytest.mark.parametrize("options", [dict(sort_driver=1), dict(sort_driver=0), dict(sort_driver=1, emit_items=2), dict(sort_driver=0, emit_items=2)],
                         ids=["onesweep", "rocprim", "onesweep-emit2", "rocprim-emit2"])
@pytest.mark.parametrize("scene", sorted(SURFEL_SCENES))
def test_surfel_train_forward_backward(scene, options):
    P, W, H, seed, mu, dead = SURFEL_SCENES[scene]
    case = _dead_scene("S", P, W, H, seed, mu, dead)
    ref, gr, _ = _oracle_of(case, "S")
    res = _with_options(options, lambda: across("surfel train %s %s" % (scene, options), lambda: _raster_run("S", case[3], case[4])))
    _check_raster("S", res, ref, gr, scene)


@pytest.mark.parametrize("sort_driver", [1, 0])
@pytest.mark.parametrize("antialiasing", [False, True])
@pytest.mark.parametrize("P,W,H,dead", [(257, 96, 64, (64, 128)), (4097, 200, 136, (0, 256))])
def test_gauss_train_forward_backward(P, W, H, dead, antialiasing, sort_driver):
    case = _dead_scene("G", P, W, H, 70 + P % 7, -1.6 if P < 1000 else -3.0, dead)
    ref, gr, _ = _oracle_of(case, "G", antialiasing)
    res = _with_options(dict(sort_driver=sort_driver),
                        lambda: across("gauss train P=%d aa=%s driver=%d" % (P, antialiasing, sort_driver), lambda: _raster_run("G", case[3], case[4], antialiasing)))
    _check_raster("G", res, ref, gr, "gauss P=%d" % P)


def _forward_only(variant, kwc):
    hip = (HipSurfel if variant == "S" else HipGauss)(kwc, requires_grad=False)
    return {k: v for k, v in hip.out().items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("W,H", [(1, 1), (17, 15)])
@pytest.mark.parametrize("variant", ["S", "G"])
def test_empty_culled_and_tiny_images(variant, W, H):
    """P = 0: zero planes, as the reference returns for an empty scene.  Every Gaussian behind the camera (num_rendered = 0, the binning
    kernels run on empty lists): the colour is the background bit for bit, every other plane zero.  A live scene on the same image: the
    same bits under every pattern, every pixel of the ragged (or single-pixel) tile finite."""
    bg = np.array([0.2, 0.4, 0.6], np.float32)
    kw, _, _ = scene_kwargs(variant, 65, W, H, 90, -1.6, 1, tuple(bg))
    per_gaussian = [k for k, v in kw.items() if isinstance(v, np.ndarray) and v.shape[:1] == (65,)]
    empty = dict(kw, **{k: kw[k][:0] for k in per_gaussian})
    behind = dict(kw, means3D=kw["means3D"].copy())
    behind["means3D"][:, 2] = -np.abs(behind["means3D"][:, 2]) - 1.0
    for name, scene in (("empty", empty), ("culled", behind), ("live", kw)):
        kwc = to_cuda(scene)
        res = across("%s %s %dx%d" % (variant, name, W, H), lambda: _forward_only(variant, kwc))
        same_bits(res, name)
        for r in res:
            all_finite(r, name)
            planes = [k for k in r if k not in ("color", "radii")]
            if name != "live":
                assert all((r[k] == 0).all() for k in planes + ["radii"]), name
                np.testing.assert_array_equal(r["color"], np.broadcast_to((bg if name == "culled" else 0 * bg)[:, None, None], (3, H, W)))


@pytest.mark.parametrize("variant", ["S", "G"])
def test_everything_culled_forward_and_backward(variant):
    """num_rendered = 0 at a size with several tiles and several preprocess workgroups: the image is the background under every pattern,
    and the backward leaves exactly zero gradients in every row."""
    P, W, H = 700, 200, 136
    case = _dead_scene(variant, P, W, H, 91, -3.0, (0, P))
    res = across("%s all culled" % variant, lambda: _raster_run(variant, case[3], case[4], antialiasing=True))
    fwd, grads = (FORWARD_S, GRADS_S) if variant == "S" else (FORWARD_G, GRADS_G)
    same_bits(res, "all culled", keys=fwd + ("num_rendered", "ranges", "n_contrib", "final_T", "tiles_touched", "point_offsets") + grads)
    for r in res:
        all_finite(r, "all culled", keys=fwd + grads)
        assert int(r["num_rendered"][0]) == 0 and (r["radii"] == 0).all() and (r["ranges"] == 0).all()
        np.testing.assert_array_equal(r["color"], np.broadcast_to(case[0]["bg"][:, None, None], (3, H, W)))
        assert all((r[k] == 0).all() for k in grads)


@pytest.mark.parametrize("refl", [False, True])
def test_inference_forward(refl):
    """rasterize_gaussians_eval: every plane the same bits under every pattern, and the bits of the corresponding training plane."""
    import test_gpu_eval_forward as EF
    from diff_surfel_rasterization import _C
    s = EF._scene(4097, 200, 136, seed=11)
    a = EF._args(s)
    r = EF._refl(s) if refl else None
    no_mask = torch.zeros(0, dtype=torch.bool, device="cuda")

    def run():
        tr = _C.rasterize_gaussians(*a[:2], no_mask, *a[2:], refl=None if r is None else dict(r, keys=False))
        ev = _C.rasterize_gaussians_eval(*a, refl=r)
        out = dict(n=np.array([ev[0], tr[0]]), color=npy(ev[1]), alpha=npy(ev[2]), normal=npy(ev[3]), refl_map=npy(ev[4]), radii=npy(ev[5]),
                   t_color=npy(tr[1]), t_others=npy(tr[2]), t_refl_map=npy(tr[7]), t_radii=npy(tr[3]), t_weights=npy(tr[8]))
        if refl:
            out.update(final=npy(ev[6]), refl_color=npy(ev[7]), nworld=npy(ev[8]), t_final=npy(tr[9]), t_refl_color=npy(tr[10]), t_nworld=npy(tr[11]))
        return out
    res = across("rasterize_gaussians_eval refl=%s" % refl, run)
    same_bits(res, "eval forward")
    for r_ in res:
        all_finite(r_, "eval forward")
        assert r_["n"][0] == r_["n"][1] > 0
        pairs = [("color", r_["t_color"]), ("alpha", r_["t_others"][1:2]), ("refl_map", r_["t_refl_map"]), ("radii", r_["t_radii"])]
        pairs += [("final", r_["t_final"]), ("refl_color", r_["t_refl_color"]), ("nworld", r_["t_nworld"])] if refl else [("normal", r_["t_others"][2:5])]
        for k, t in pairs:
            np.testing.assert_array_equal(poison.u32(r_[k]), poison.u32(t), err_msg=k)


# =============================================================================================== reflection: two-node and fused
SORT_SHAPE_SIZES = [104, 105, 209, 210, 418, 419]        # where the texel-id sort changes shape (tests/test_gpu_refl_seams.py, SIZES)
POISONED_PATHS = ("forward_keys", "backward_keys", "atomics", "async_tail")      # (c_abi allocates in the test, not in the package)


@pytest.mark.parametrize("L", SORT_SHAPE_SIZES)
def test_deferred_reflection_at_the_sort_shapes(L):
    """The two-node deferred reflection with forward keys on and off, the sorted-footprint and the atomics backward and the side-stream
    tail, on the seam image of helpers_refl.py: every check of that file (forward planes, pixel gradients, cubemap and fail-value gradients,
    its tolerances) under each pattern; forward planes and per-pixel gradients the same bits under every pattern."""
    import helpers_refl as R
    inp = R.seam_inputs(L, seed=L)
    ref = R.reference_run(inp)
    env = R.envelope(inp, ref)
    fails = []
    for path in POISONED_PATHS:
        res = across("deferred_reflection L=%d %s" % (L, path), lambda: (R.hip_run(inp, path, False), R.hip_run(inp, path, True)))
        for k in (0, 1):
            same_bits([r[k] for r in res], path, keys=("final", "refl", "nworld", "g_nv", "g_base", "g_s"))
        for pattern, got in zip(PATTERNS, res):
            all_finite(got[0], path)
            all_finite(got[1], path)
            fails += R.check_path(inp, ref, env, got, "%s/0x%02X" % (path, pattern))[1]
    assert not fails, fails


@pytest.mark.parametrize("async_tail", [False, True])
@pytest.mark.parametrize("L", [16, 128, 210, 419])
def test_fused_node_on_the_mirror_scene(L, async_tail):
    """rasterize_reflect (reflection forward in the tile kernel's epilogue, keys, with async_tail the early sort into the backward's
    scratch) against the float64 chain with helpers_refl.py's checks under each pattern; its planes the same bits under every pattern.
    L = 16 and 128 take the early sort's 8- and 9-bit digit shapes, 210 the 10-bit shape and 419 the three 8-bit passes, where the
    early sort clears its own look-back region."""
    import helpers_refl as R
    res = across("rasterize_reflect mirror L=%d async_tail=%s" % (L, async_tail), lambda: R.mirror_case("vertex", L, async_tail))
    for k in (0, 1):
        same_bits([got[k] for _, got in res], "mirror", keys=("final", "refl", "nworld", "nv", "base", "strength", "g_nv", "g_base", "g_s"))
    fails = []
    for pattern, (inp, got) in zip(PATTERNS, res):
        all_finite(got[0], "mirror")
        ref = R.reference_run(inp)
        fails += R.check_path(inp, ref, R.envelope(inp, ref), got, "mirror/0x%02X" % pattern)[1]
    assert not fails, fails


_fused_refs = {}


def _fused_scene(P):
    """Scene and the two-node path's outputs and gradients, computed once outside any poisoned scope."""
    import test_gpu_fused as F
    if P not in _fused_refs:
        W, H = 200, 136
        src, mask, cam, ct, bg = F._scene(4097, 43, -3.0, 32, W, H)
        if P == 0:
            src, mask = {k: (v if k in ("cubemap", "fail") else v[:0]) for k, v in src.items()}, mask[:0]
        ups = F._upstream(H, W, 4, ("final", "allmap") if P else ("final", "allmap", "refl_color"))
        p = {k: v.clone().requires_grad_(True) for k, v in src.items()}
        out, g2d = F._run(False, p, mask, cam, ct, W, H, bg, ups)
        torch.cuda.synchronize()
        _fused_refs[P] = (src, mask, cam, ct, bg, W, H, ups, {k: npy(v) for k, v in out.items()}, {k: npy(p[k].grad) for k in F.PARAMS})
    return _fused_refs[P]


@pytest.mark.parametrize("binned", [True, False], ids=["sorted", "atomics"])
@pytest.mark.parametrize("forward_keys", [True, False])
def test_fused_equals_the_two_node_path(forward_keys, binned, monkeypatch):
    """gaussian_renderer.rasterize_reflect under each pattern against the two-node path run once without poison, as tests/test_gpu_fused.py
    compares them: the rasterizer's own outputs the same bits, reflection outputs to 5e-6, every gradient to 5e-5 of its maximum."""
    import gaussian_renderer as gr
    import test_gpu_fused as F
    monkeypatch.setattr(gr, "REFLECTION_FORWARD_KEYS", forward_keys)
    monkeypatch.setattr(gr, "REFLECTION_BACKWARD_BINNED", binned)
    src, mask, cam, ct, bg, W, H, ups, out_ref, g_ref = _fused_scene(4097)

    def run():
        p = {k: v.clone().requires_grad_(True) for k, v in src.items()}
        out, g2d = F._run(True, p, mask, cam, ct, W, H, bg, ups)
        r = {k: npy(v) for k, v in out.items()}
        r.update({"g_" + k: npy(p[k].grad) for k in F.PARAMS})
        return r
    res = across("rasterize_reflect keys=%s binned=%s" % (forward_keys, binned), run)
    same_bits(res, "fused", keys=("final", "refl_color", "nworld", "base", "radii", "allmap", "refl_map", "gw"))
    for r in res:
        all_finite(r, "fused")
        for k in ("base", "radii", "allmap", "refl_map", "gw"):
            np.testing.assert_array_equal(poison.u32(r[k]), poison.u32(out_ref[k]), err_msg=k)
        for k in ("final", "refl_color", "nworld"):
            assert np.abs(r[k] - out_ref[k]).max() <= 5e-6, k
        for k in F.PARAMS:
            assert k == "fail" or np.abs(g_ref[k]).max() > 0, k
            assert rel_maxnorm(r["g_" + k], g_ref[k]) <= 5e-5, k


@pytest.mark.parametrize("async_tail", [False, True])
@pytest.mark.parametrize("P", [4097, 0])
def test_fused_with_sinks_and_the_early_sort(P, async_tail):
    """Both gradient sinks (NaN-filled flat buffer), the texel-gradient tail on the side stream and, with it, the forward's early sort of
    the keys into the scratch the backward takes over; P = 0 takes the same tail through the stand-alone pixel pass.  Every sunk gradient
    finite and within 5e-5 of the two-node path's under each pattern."""
    import _gsr
    import test_gpu_fused as F
    from gsr_dist import FlatGrads
    src, mask, cam, ct, bg, W, H, ups, out_ref, g_ref = _fused_scene(P)
    checked = F.PARAMS if P else ("cubemap", "fail")

    def run():
        p = {k: v.clone().requires_grad_(True) for k, v in src.items()}
        fg = FlatGrads(p)
        fg.flat.fill_(float("nan"))
        out, _ = F._run(True, p, mask, cam, ct, W, H, bg, ups, raster_sink=fg.sink(), refl_sink=fg.sink(names=("cubemap", "fail")), accumulate=False,
                        async_tail=async_tail)
        _gsr.side_join()
        torch.cuda.synchronize()
        r = {k: npy(out[k]) for k in ("final", "refl_color", "nworld", "base", "allmap", "refl_map")}
        r.update({"g_" + k: npy(fg.view(k)) for k in checked})
        return r
    res = across("rasterize_reflect sinks P=%d async_tail=%s" % (P, async_tail), run)
    same_bits(res, "fused sinks", keys=("final", "refl_color", "nworld", "base", "allmap", "refl_map"))
    for r in res:
        all_finite(r, "fused sinks")
        for k in checked:
            assert k == "fail" or np.abs(g_ref[k]).max() > 0, k
            assert rel_maxnorm(r["g_" + k], g_ref[k]) <= 5e-5, k
