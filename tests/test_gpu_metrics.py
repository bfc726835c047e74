"""The evaluation metrics kernels (csrc/gsr_metrics.hip) and their Python layers (gsr_eval.py, utils/image_utils.py,
utils/mae_utils.py) on the GPU against the float64 references and bounds of tests/metrics_ref.py: every presentation variant at the
shapes where a 32 x 32 tile with a 42 x 42 halo goes wrong, the 8-bit images bit for bit against torch's float32 chain on the CPU,
the table's rows, and evaluate_views against render_fast composed with the references.  Every test prints its worst error / bound."""
import numpy as np
import pytest
import torch

import loss_bounds as LB
import metrics_ref as MR

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_image(v, g, kw, want_u8=False, table=None, row=0):
    """One gsr_image_metrics call through MetricsTable on float32 numpy inputs; returns (row as numpy, img_u8, gt_u8)."""
    from gsr_eval import MetricsTable
    t = MetricsTable(1, "cuda") if table is None else table
    u8 = (torch.full(v.shape, 77, dtype=torch.uint8, device="cuda"), torch.full(v.shape, 77, dtype=torch.uint8, device="cuda")) if want_u8 else (None, None)
    t.image(row, _dev(v), _dev(g), clamp=kw.get("clamp", False), alpha=_dev(kw.get("alpha")), gt_mask=_dev(kw.get("gt_mask")),
            background=_dev(kw.get("background")), quantize8=kw.get("quantize", False), img_u8=u8[0], gt_u8=u8[1])
    r = t.result()[row]
    return r, (None if u8[0] is None else u8[0].cpu().numpy()), (None if u8[1] is None else u8[1].cpu().numpy())


def check_image(v, g, kw, what):
    pv, pg, lv, lg = MR.present(v, g, **kw)
    ref, bnd = MR.image_sums_reference(pv, pg)
    row, u8v, u8g = run_image(v, g, kw, want_u8=bool(kw.get("quantize")))
    q = {k: MR.check_scalar(row[i], ref[k], bnd[k], f"{what} {k}") for i, k in enumerate(("sse", "sad", "ssim"))}
    assert row[3] == v.size
    if kw.get("quantize"):
        _, _, tlv, tlg = MR.torch_present(v, g, **kw)
        np.testing.assert_array_equal(u8v, tlv, err_msg=f"{what}: rendered image, 8 bit")
        np.testing.assert_array_equal(u8g, tlg, err_msg=f"{what}: ground truth, 8 bit")
        np.testing.assert_array_equal(lv, tlv)
    print(f"measured {what}: sse {q['sse']:.3f} sad {q['sad']:.3f} ssim {q['ssim']:.3f} of the bound")
    return row, ref, bnd


@pytest.mark.parametrize("variant", MR.VARIANTS)
@pytest.mark.parametrize("family", MR.IMAGE_FAMILIES)
def test_image_sums_and_8bit_images(family, variant):
    for i, shape in enumerate(MR.IMAGE_SHAPES):
        v, g = MR.image_pair(family, shape, 10 + i)
        kw = MR.presentation_inputs(variant, shape, 10 + i)
        row, ref, bnd = check_image(v, g, kw, f"{family} {variant} {shape}")
        if family == "identical" and variant in ("none", "clamp"):
            assert row[0] == 0.0 and row[1] == 0.0
            assert abs(row[2] / row[3] - 1.0) <= bnd["ssim"] / row[3]


@pytest.mark.parametrize("family, variant", [("uniform", "clamp_composite_quantize")])
def test_full_size(family, variant):
    v, g = MR.image_pair(family, MR.FULL_SIZE, 3)
    check_image(v, g, MR.presentation_inputs(variant, MR.FULL_SIZE, 3), f"{family} {variant} full size")


def test_quantiser_edges_every_level_bit_for_bit():
    """The whole edge set in one image, quantisation alone: the 8-bit outputs are torch's, level for level."""
    e = MR.quantizer_edge_values()
    n = 3 * 29 * 31
    assert n >= e.size
    v = np.resize(e, n).reshape(3, 29, 31).astype(np.float32)
    g = np.resize(e[::-1], n).reshape(3, 29, 31).astype(np.float32)
    kw = dict(quantize=True)
    _, u8v, u8g = run_image(v, g, kw, want_u8=True)
    _, _, tlv, tlg = MR.torch_present(v, g, **kw)
    np.testing.assert_array_equal(u8v, tlv)
    np.testing.assert_array_equal(u8g, tlg)
    assert set(np.unique(u8v)) == set(range(256))


@pytest.mark.parametrize("shape", [(3, 33, 31), (3, 43, 75), (1, 64, 96)])
def test_without_presentation_agrees_with_the_training_loss(shape):
    """Presentation off: sum |v - g| and sum ssim against gsr_ssim_l1_forward's two sums, each within the same float64 bounds."""
    from _gsr import check, lib, stream_ptr
    v, g = MR.image_pair("uniform", shape, 21)
    ref, bnd = MR.image_sums_reference(v.astype(np.float64), g.astype(np.float64))
    row, _, _ = run_image(v, g, {})
    X, Y = _dev(v), _dev(g)
    C, H, W = shape
    sums = torch.full((2,), float("nan"), device="cuda")
    scratch = torch.empty(max(1, int(lib.gsr_ssim_l1_scratch_floats(C, H, W))), device="cuda")
    check(lib.gsr_ssim_l1_forward(X.data_ptr(), Y.data_ptr(), C, H, W, LB.C1, LB.C2, sums.data_ptr(), scratch.data_ptr(), None, None, None, None,
                                  stream_ptr(X.device)), "gsr_ssim_l1_forward")
    s = sums.cpu().numpy().astype(np.float64)
    for got, k in ((row[1], "sad"), (s[0], "sad"), (row[2], "ssim"), (s[1], "ssim")):
        MR.check_scalar(got, ref[k], bnd[k], f"{shape} {k}")
    assert abs(row[1] - s[0]) <= 2 * bnd["sad"] and abs(row[2] - s[1]) <= 2 * bnd["ssim"]


def test_identical_images_and_psnr():
    """SSE exactly 0, psnr = inf, mean SSIM = 1 within its bound; and the known answers of tests/test_metrics_ref.py on the device."""
    from utils.image_utils import mse, psnr
    v, _ = MR.image_pair("uniform", (3, 43, 75), 4)
    ref, bnd = MR.image_sums_reference(v.astype(np.float64), v.astype(np.float64))
    row, _, _ = run_image(v, v.copy(), {})
    assert row[0] == 0.0 and row[1] == 0.0
    assert abs(row[2] / row[3] - 1.0) <= bnd["ssim"] / row[3]
    a = torch.zeros(3, 1, 33, 40, device="cuda")
    b = a.clone()
    b[0] += 0.1
    b[1] += 0.5
    b[2, 0, 0, 0] = 1.0
    with torch.no_grad():
        m, p, pi = mse(a, b), psnr(a, b), psnr(a, a)
    assert m.shape == (3, 1) and p.shape == (3, 1) and m.dtype == torch.float32
    np.testing.assert_allclose(m[:, 0].cpu().numpy(), [0.01, 0.25, 1.0 / 1320.0], rtol=1e-6)
    np.testing.assert_allclose(p[:, 0].cpu().numpy(), [20.0, 20.0 * np.log10(2.0), 10.0 * np.log10(1320.0)], rtol=1e-5)
    assert torch.isinf(pi).all() and (pi > 0).all()
    # a gradient required: the torch expression, differentiable, same value
    x = a.clone().requires_grad_(True)
    pg = psnr(x, b)
    assert pg.requires_grad
    np.testing.assert_allclose(pg.detach().cpu().numpy(), p.cpu().numpy(), rtol=1e-5)


def test_table_rows_on_a_side_stream_are_reproducible():
    """Five views into rows 0..4 of a 7-row table on a non-default stream: rows 5 and 6 keep their sentinel, a second run gives the
    same bits, and every row is its view's."""
    from gsr_eval import MetricsTable
    shape = (3, 43, 75)
    pairs = [MR.image_pair("uniform", shape, 30 + i) for i in range(5)]
    kws = [MR.presentation_inputs(MR.VARIANTS[i % 4], shape, 30 + i) for i in range(5)]
    stream = torch.cuda.Stream()
    runs = []
    for _ in range(2):
        table = MetricsTable(7, "cuda")
        table.rows.fill_(-123.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for i, ((v, g), kw) in enumerate(zip(pairs, kws)):
                table.image(i, _dev(v), _dev(g), clamp=kw.get("clamp", False), alpha=_dev(kw.get("alpha")), gt_mask=_dev(kw.get("gt_mask")),
                            background=_dev(kw.get("background")), quantize8=kw.get("quantize", False))
            stream.synchronize()
        runs.append(table.result())
    assert (runs[0][5:] == -123.0).all()
    assert runs[0].tobytes() == runs[1].tobytes()
    for i, ((v, g), kw) in enumerate(zip(pairs, kws)):
        pv, pg, _, _ = MR.present(v, g, **kw)
        ref, bnd = MR.image_sums_reference(pv, pg)
        for j, k in enumerate(("sse", "sad", "ssim")):
            MR.check_scalar(runs[0][i, j], ref[k], bnd[k], f"row {i} {k}")


# --------------------------------------------------------------------------------------------------------------- normal MAE
def check_mae(p, g, what, **div):
    from gsr_eval import MetricsTable
    ang, bound, ambiguous = MR.angular_error_reference(p, g, **div)
    assert not ambiguous.any()
    t = MetricsTable(1, "cuda")
    emap = torch.full(p.shape[1:], 5.0, device="cuda")
    t.normals(0, _dev(p), _dev(g), pred_divisor=div.get("pred_divisor", 1.0), gt_divisor=div.get("gt_divisor", 1.0), error_map=emap)
    row = t.result()[0]
    q_map = LB.check(emap.cpu().numpy(), ang, bound, what=f"{what} map")         # NaN exactly where the reference has it
    s, valid, invalid, b = MR.angle_sum_reference(ang, bound)
    assert (row[1], row[2], row[3]) == (valid, invalid, ang.size), what
    q_sum = MR.check_scalar(row[0], s, b, f"{what} sum")
    print(f"measured {what}: angle {q_map:.3f} sum {q_sum:.3f} of the bound")
    return row, ang


@pytest.mark.parametrize("family", MR.MAE_FAMILIES)
def test_normal_mae(family):
    for i, (H, W) in enumerate(MR.MAE_SHAPES):
        p, g = MR.normal_pair(family, H, W, 50 + i)
        row, ang = check_mae(p, g, f"{family} {H}x{W}")
        if family == "identical":
            assert row[0] / row[1] <= 0.1
        if family == "opposite":
            assert row[0] / row[1] >= 179.9
        if family in ("degenerate", "eps_straddle") and H * W > 1:
            assert row[1] > 0 and row[2] > 0


def test_normal_mae_full_size():
    p, g = MR.normal_pair("degenerate", 1080, 1920, 6)
    check_mae(p, g, "degenerate 1080p")


def test_compute_mae_and_angular_error_map_as_the_reference_calls_them():
    """The recorded reference vectors through the public functions: 0..255 and 0..65535 inputs rescaled by what they hold, the mean NaN
    as soon as one pixel is invalid."""
    from utils.mae_utils import angular_error_map, compute_mae
    z = np.load(MR.GOLDEN)
    for name in ("scaled_a", "scaled_b", "unit_range"):
        p, g, out = z[f"mae_{name}_pred"], z[f"mae_{name}_gt"], float(z[f"mae_{name}_out"])
        dp, dg = (255.0 if p.max() > 1.0 else 1.0), (65535.0 if g.max() > 1.0 else 1.0)
        ang, bound, _ = MR.angular_error_reference(p[0], g[0], pred_divisor=dp, gt_divisor=dg)
        s, valid, invalid, b = MR.angle_sum_reference(ang, bound)
        got = compute_mae(_dev(p), _dev(g))
        assert got.dim() == 0 and got.dtype == torch.float32
        assert abs(float(got) - s / valid) <= b / valid + 2 * MR.U * s / valid
        assert abs(float(got) - out) <= 2 * (b / valid + 2 * MR.U * s / valid)
    for family in MR.MAE_FAMILIES:
        p, g, out = z[f"map_{family}_pred"], z[f"map_{family}_gt"], z[f"map_{family}_out"]
        ang, bound, _ = MR.angular_error_reference(p, g)
        got = angular_error_map(_dev(p), _dev(g)).cpu().numpy()
        assert got.shape == out.shape and (np.isnan(got) == np.isnan(out)).all()
        print(f"ratio angle map {family}: {LB.check(got, ang, bound, what=family):.3f}")
    p, g = z["map_degenerate_pred"], z["map_degenerate_gt"]
    assert torch.isnan(compute_mae(_dev(p[None]), _dev(g[None])))


# ------------------------------------------------------------------------------------------------------------ evaluate_views
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("mu", [-3.0, -1.0])
def test_evaluate_views(masks, mu):
    """Three 64 x 48 views of a small scene: evaluate_views against render_fast composed with the float64 references.  Small surfels
    (mu = -3) leave pixels uncovered, whose zero normal makes a view's MAE NaN as in the reference; large ones (mu = -1) cover every
    pixel, so the finite MAE per view and its mean are held to their bounds."""
    from gaussian_renderer import render_fast
    from gsr_eval import MetricsTable, evaluate_views
    from test_gpu_dropin import _Pipe, _model, _scene, _view
    from helpers import S
    W, H = 64, 48
    t, env = _scene(3000, 5, mu, 16)
    PC = _model(t, env)
    bg = torch.tensor([0.1, 0.95, 0.3], device="cuda")
    rs = np.random.RandomState(8)
    views, normals = [], []
    for i, eye in enumerate(((0.4, -0.3, -1.0), (-0.5, 0.2, -1.2), (0.0, 0.6, -0.8))):
        View = _view(S.look_at_camera(W, H, eye=eye, target=(0, 0, 5)), W, H)
        View.original_image = torch.from_numpy(rs.rand(3, H, W).astype(np.float32)).cuda()
        View.gt_alpha_mask = torch.from_numpy((rs.rand(1, H, W) < 0.8).astype(np.float32)).cuda() if masks else None
        views.append(View)
        normals.append(torch.from_numpy(MR.normal_pair("random", H, W, 60 + i)[1]).cuda())
    out = evaluate_views(views, PC, _Pipe, bg, gt_normals=normals, keep_images=True)
    assert set(out) == {"PSNR", "SSIM", "MAE", "per_view", "images"} and set(out["per_view"]) == {"PSNR", "SSIM", "MAE"}
    psnrs, ssims, maes, b_psnr, b_ssim, b_mae = [], [], [], [], [], []
    for i, View in enumerate(views):
        with torch.no_grad():
            pkg = render_fast(View, PC, _Pipe, bg)
        kw = dict(clamp=True, quantize=True)
        if masks:
            kw.update(alpha=pkg["rend_alpha"].cpu().numpy()[0], gt_mask=View.gt_alpha_mask.cpu().numpy()[0], background=bg.cpu().numpy())
        v, g = pkg["render"].cpu().numpy(), View.original_image.cpu().numpy()
        pv, pg, _, _ = MR.present(v, g, **kw)
        _, _, tlv, tlg = MR.torch_present(v, g, **kw)
        np.testing.assert_array_equal(out["images"][i][0].cpu().numpy(), tlv)
        np.testing.assert_array_equal(out["images"][i][1].cpu().numpy(), tlg)
        ref, bnd = MR.image_sums_reference(pv, pg)
        n = v.size
        psnrs.append(MR.psnr(ref["sse"], n))
        ssims.append(ref["ssim"] / n)
        b_psnr.append(MR.psnr_bound(ref["sse"], bnd["sse"]))
        b_ssim.append(bnd["ssim"] / n)
        assert abs(out["per_view"]["PSNR"][i] - psnrs[-1]) <= b_psnr[-1]
        assert abs(out["per_view"]["SSIM"][i] - ssims[-1]) <= b_ssim[-1]
        ang, bound, amb = MR.angular_error_reference(pkg["rend_normal"].cpu().numpy(), normals[i].cpu().numpy())
        s, valid, invalid, b = MR.angle_sum_reference(ang, bound)
        assert not amb.any()
        nt = MetricsTable(1, "cuda")      # the row evaluate_views read: sum and counts, also where the view's mean is NaN
        nt.normals(0, pkg["rend_normal"], normals[i])
        nrow = nt.result()[0]
        assert (nrow[1], nrow[2]) == (valid, invalid)
        MR.check_scalar(nrow[0], s, b, f"view {i} angle sum")
        if invalid:                       # a pixel no surfel covers has a zero normal: the reference's mean is NaN then
            assert np.isnan(out["per_view"]["MAE"][i])
            maes.append(np.nan)
        else:
            assert abs(out["per_view"]["MAE"][i] - s / valid) <= b / valid
            maes.append(s / valid)
            b_mae.append(b / valid)
    # a mean of the per-view values is off by at most the mean of their bounds
    assert abs(out["PSNR"] - np.mean(psnrs)) <= np.mean(b_psnr) and abs(out["SSIM"] - np.mean(ssims)) <= np.mean(b_ssim)
    if mu == -1.0:
        assert len(b_mae) == 3, "the covering scene must give every view a finite MAE"
    assert np.isnan(out["MAE"]) if np.isnan(maes).any() else abs(out["MAE"] - np.mean(maes)) <= np.mean(b_mae)
    plain = evaluate_views(views, PC, _Pipe, bg, quantize8=False)
    assert set(plain) == {"PSNR", "SSIM", "per_view"}
    assert all(abs(a - b) < 0.5 for a, b in zip(plain["per_view"]["PSNR"], out["per_view"]["PSNR"]))


# ------------------------------------------------------------------------------------------------------ callers and contracts
def test_psnr_as_the_training_loop_calls_it():
    """train.py's test iteration: psnr(image, gt_image).mean().double() under no_grad on [3, H, W] device tensors.  Dim 0 is the batch
    (the reference's view(img1.shape[0], -1)): a [3, 1] result, one value per channel, here from the kernel; other ranks likewise; what
    the kernel cannot read as it is goes through the reference's expression and gives the same numbers."""
    from utils.image_utils import mse, psnr
    v, g = MR.image_pair("uniform", (3, 43, 75), 12)
    X, Y = _dev(v), _dev(g)
    d = v.astype(np.float64) - g.astype(np.float64)
    want_mse = (d * d).reshape(3, -1).mean(1)
    want = 20 * np.log10(1.0 / np.sqrt(want_mse))
    with torch.no_grad():
        p, m = psnr(X, Y), mse(X, Y)
        scalar = psnr(X, Y).mean().double()
    assert p.shape == (3, 1) and m.shape == (3, 1) and p.dtype == torch.float32
    np.testing.assert_allclose(m[:, 0].cpu().numpy(), want_mse, rtol=2e-7)
    np.testing.assert_allclose(p[:, 0].cpu().numpy(), want, rtol=2e-7)
    assert scalar.dtype == torch.float64 and abs(float(scalar) - want.mean()) <= 1e-5
    with torch.no_grad():
        cases = ((X[0], Y[0]), (X[0, 0, :64], Y[0, 0, :64]), (X.reshape(3, 1, 5, 43, 15), Y.reshape(3, 1, 5, 43, 15)))      # 2-D, 1-D, 5-D
        for a, b in cases:
            got, ref = mse(a, b), (((a - b)) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
            assert got.shape == ref.shape == (a.shape[0], 1)
            np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-12)
        # float64 inputs and shapes that only broadcast: the reference's expression, as there
        p64 = psnr(X.double(), Y.double())
        assert p64.dtype == torch.float64 and p64.shape == (3, 1)
        np.testing.assert_allclose(p64[:, 0].cpu().numpy(), want, rtol=1e-12)
        pb = psnr(X, Y[:, :1, :])
        assert pb.shape == (3, 1) and torch.isfinite(pb).all()


def test_composite_keeps_its_separate_roundings():
    """The pixels of metrics_ref.COMPOSITE_EDGES: a composite with either product folded into a fused multiply-add lands on another
    8-bit level there (tests/test_metrics_ref.py shows it), so these levels hold the kernel's four separate roundings, for the render
    (alpha) and for the ground truth (mask)."""
    img, alpha, bg = MR.composite_edge_image()
    kw = dict(alpha=alpha, gt_mask=alpha, background=bg, quantize=True)
    _, u8v, u8g = run_image(img, img.copy(), kw, want_u8=True)
    _, _, tlv, tlg = MR.torch_present(img, img, **kw)
    np.testing.assert_array_equal(u8v, tlv)
    np.testing.assert_array_equal(u8g, tlg)
    t64, a64 = img.astype(np.float64), alpha.astype(np.float64)
    for i, (_, _, c) in enumerate(MR.COMPOSITE_EDGES):
        other = MR.quantize_levels(MR.composite_contracted(t64, a64, bg, 0 if i < 4 else 1))
        assert u8v[c, i // 4, i % 4] != other[c, i // 4, i % 4] and u8g[c, i // 4, i % 4] != other[c, i // 4, i % 4]


def test_tensors_must_live_on_the_tables_device():
    from gsr_eval import MetricsTable
    t = MetricsTable(1, "cuda")
    x = torch.zeros(3, 4, 4, device="cuda")
    with pytest.raises(ValueError, match="table's device"):
        t.normals(0, x, x, error_map=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="table's device"):
        t.image(0, x, x, alpha=torch.zeros(4, 4), background=torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError, match="table's device"):
        t.image(0, x, x, quantize8=True, img_u8=torch.zeros(3, 4, 4, dtype=torch.uint8))
    assert np.isnan(t.result()).all()          # nothing ran
