"""The references and error bounds of tests/loss_front_bounds.py, checked on the CPU, and the argument validation of the new
C entries (which runs before any device call):
  * the float64 recipe (composites in numpy, the oracle on them, the chain rule in numpy) against float64 torch autograd of
    the literal train.py:158-159, 167-174 expression;
  * a float32 evaluation of the whole chain stays inside the bounds for every content family, plane kind and background;
  * the bounds are not vacuous and reject an error placed just outside them;
  * the map-gradient restatement with a constant upstream gradient is the oracle's SSIM backward;
  * GSR_E_INVALID for every argument error include/gsr_hip.h lists."""
import numpy as np
import pytest
import torch

import loss_bounds as LB
import loss_front_bounds as FB
from oracle import oracle as orc

W_L1, W_SSIM = 0.8, -0.2


def _literal_loss(rgb, alpha, gt, mask, bg, lam):
    """train.py:158-159, 167-174 in torch float64: composites, l1_loss, the reference's _ssim with its float32 window."""
    import torch.nn.functional as F
    C = rgb.shape[0]
    g1 = torch.from_numpy(LB.window1d().astype(np.float32))
    window = torch.outer(g1, g1).to(torch.float64)[None, None].expand(C, 1, 11, 11).contiguous()
    gt_image = gt * mask + (1 - mask) * bg[:, None, None]
    image = rgb * alpha + (1 - alpha) * bg[:, None, None]
    l1 = (image - gt_image).abs().mean()
    conv = lambda t: F.conv2d(t[None], window, padding=5, groups=C)[0]
    mu1, mu2 = conv(image), conv(gt_image)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = conv(image * image) - mu1_sq, conv(gt_image * gt_image) - mu2_sq, conv(image * gt_image) - mu1_mu2
    ssim_map = ((2 * mu1_mu2 + LB.C1) * (2 * sigma12 + LB.C2)) / ((mu1_sq + mu2_sq + LB.C1) * (sigma1_sq + sigma2_sq + LB.C2))
    return (1.0 - lam) * l1 + lam * (1.0 - ssim_map.mean()), (image - gt_image).abs().sum(), ssim_map.sum()


@pytest.mark.parametrize("shape,alpha_kind,mask_kind", [((3, 37, 43), "outside", "soft"), ((2, 33, 65), "regions", "binary"), ((5, 11, 6), "ramp", "soft")])
def test_recipe_equals_float64_autograd_of_the_literal_expression(shape, alpha_kind, mask_kind):
    case = FB.front_case("uniform", shape, 5, (True, True), alpha_kind, mask_kind)
    n, lam = case["rgb"].size, 0.2
    ref, _ = FB.front_reference(case, (1.0 - lam) / n, -lam / n)
    t = {k: torch.from_numpy(case[k].astype(np.float64)) for k in ("rgb", "alpha", "gt", "mask", "bg")}
    t["rgb"].requires_grad_(True)
    t["alpha"].requires_grad_(True)
    loss, s_l1, s_ss = _literal_loss(t["rgb"], t["alpha"][None], t["gt"], t["mask"][None], t["bg"], lam)
    loss.backward()
    s_l1, s_ss = s_l1.item(), s_ss.item()
    assert abs(s_l1 - ref["l1"]) <= 1e-4 and abs(s_ss - ref["ssim"]) <= 1e-4
    # (gradients of the SUMS' weights scaled back to magnitudes of order 1, as the issue's measurement: weights w / n times n)
    assert np.abs(t["rgb"].grad.numpy() - ref["drgb"]).max() * n <= 1e-6
    assert np.abs(t["alpha"].grad.numpy() - ref["dalpha"]).max() * n <= 1e-6


def _cases(family, k0=0):
    """Three shapes per family; every combination of planes given, every alpha and mask kind and background appears."""
    for k, shape in enumerate([(3, 37, 65), (2, 64, 33), (1, 6, 11)]):
        i = k0 + k
        yield FB.front_case(family, shape, 1 + i, FB.COMBOS[i % 4], FB.ALPHA_KINDS[i % 4], FB.MASK_KINDS[i % 2], FB.BACKGROUNDS[i % 3]), shape


@pytest.mark.parametrize("family", LB.FAMILIES)
def test_bounds_hold_for_a_float32_evaluation_of_the_chain(family):
    for k0 in (0, 1, 2, 3):
        for case, shape in _cases(family, k0 + LB.FAMILIES.index(family)):
            ref, bnd = FB.front_reference(case, W_L1, W_SSIM)
            got = FB.chain_f32(case, W_L1, W_SSIM)
            FB.check_front(got, ref, bnd, f"{family} {shape} {k0}")


def test_composite_error_is_zero_exactly_where_the_composite_is_exact():
    rgb, _ = LB.loss_pair("uniform", (3, 40, 70), 3)
    a = FB.alpha_plane("regions", 40, 70, 3)
    bg = np.array(FB.BACKGROUNDS[2], np.float32)
    v, d_v = FB.composite(rgb, a, bg)
    exact = (a == 0) | (a == 1)
    assert exact.any() and (~exact).any()
    assert (d_v[:, exact] == 0).all() and (d_v[:, ~exact] > 0).all()
    assert (v[:, a == 0] == bg.astype(np.float64)[:, None]).all() and (v[:, a == 1] == rgb[:, a == 1]).all()
    # both float32 arrangements of the composite stay within the error: unfused, and with one fused multiply-add
    one = np.float32(1)
    unfused = rgb * a[None] + (one - a[None]) * bg[:, None, None]
    fused = (rgb.astype(np.float64) * a[None] + ((one - a[None]) * bg[:, None, None]).astype(np.float64)).astype(np.float32)
    for got in (unfused, fused):
        assert (np.abs(got - v) <= LB.U * d_v).all()


def test_a_near_tie_is_refused():
    case = FB.front_case("uniform", (1, 8, 9), 1, (True, True), "noise", "soft")
    case["gt"] = case["rgb"].copy()
    case["mask"] = case["alpha"].copy()          # v == g in float64, neither exact
    with pytest.raises(AssertionError, match="near ties"):
        FB.front_reference(case, W_L1, W_SSIM)


def test_bounds_are_not_vacuous_and_reject_an_error_just_outside():
    case = FB.front_case("uniform", (3, 64, 96), 2, (True, True), "noise", "soft")
    ref, bnd = FB.front_reference(case, W_L1, W_SSIM)
    # the composites' own errors add a modest share to what the plain loss allows on the same (rounded) composites; the
    # alpha gradient is a signed sum of C such terms
    v, _ = FB.composite(case["rgb"], case["alpha"], case["bg"])
    g, _ = FB.composite(case["gt"], case["mask"], case["bg"])
    ref0, bnd0 = LB.ssim_reference(v.astype(np.float32), g.astype(np.float32), W_L1, W_SSIM)
    plain = np.median(bnd0["grad"] / np.abs(ref0["grad"]))
    assert plain < np.median(bnd["drgb"] / np.abs(ref["drgb"])) < 1.5 * plain < 5e-3
    assert np.median(bnd["dalpha"] / np.abs(ref["dalpha"])) < 1e-2
    assert bnd["l1"] < 1e-5 * ref["l1"] and bnd["ssim"] < 1e-3 * abs(ref["ssim"])
    for k, idx in (("drgb", (1, 17, 33)), ("dalpha", (17, 33)), ("dv", (2, 63, 0))):
        bad = ref[k].copy()
        bad[idx] += 1.01 * bnd[k][idx]
        with pytest.raises(AssertionError):
            LB.check(bad, ref[k], bnd[k], what=k)
        ok = ref[k].copy()
        ok[idx] += 0.99 * bnd[k][idx]
        LB.check(ok, ref[k], bnd[k], what=k)
    for k in ("l1", "ssim"):
        with pytest.raises(AssertionError):
            LB.check(ref[k] + 1.01 * bnd[k], ref[k], bnd[k])
    x, y = LB.loss_pair("uniform", (2, 40, 50), 3)
    G = np.random.RandomState(3).randn(2, 40, 50).astype(np.float32)
    # a positive upstream gradient keeps the 121 terms of a window coherent: the planes' own relative error (that of the map,
    # ~1e-4, through 1 / D) times the few terms of the combination; random signs cancel the value like sqrt(121) and not the bound
    ref, bnd = FB.map_grad_reference(x, y, np.abs(G))
    assert np.median(bnd / np.abs(ref)) < 2e-3
    ref, bnd = FB.map_grad_reference(x, y, G)
    assert np.median(bnd / np.abs(ref)) < 11 * 2e-3
    bad = ref.copy()
    bad[1, 17, 33] += 1.01 * bnd[1, 17, 33]
    with pytest.raises(AssertionError):
        LB.check(bad, ref, bnd)


def test_without_planes_the_bounds_are_those_of_the_plain_loss():
    """No alpha, no mask: the composites are the images, their errors zero, and the extended scheme is loss_bounds' own."""
    case = FB.front_case("lowpass", (2, 37, 43), 4, (False, False))
    ref, bnd = FB.front_reference(case, W_L1, W_SSIM)
    ref0, bnd0 = LB.ssim_reference(case["rgb"], case["gt"], W_L1, W_SSIM)
    assert ref["l1"] == ref0["l1"] and ref["ssim"] == ref0["ssim"] and np.array_equal(ref["drgb"], ref0["grad"])
    assert np.allclose(bnd["drgb"], bnd0["grad"], rtol=1e-12, atol=0) and np.isclose(bnd["l1"], bnd0["l1"], rtol=1e-12) and np.isclose(bnd["ssim"], bnd0["ssim"], rtol=1e-12)


@pytest.mark.parametrize("family", ["uniform", "hdr", "bright_flat", "steps"])
def test_map_gradient_restatement_with_a_constant_upstream_is_the_oracle_backward(family):
    w = 0.37
    for shape in [(3, 37, 65), (1, 6, 11), (2, 32, 33)]:
        x, y = LB.loss_pair(family, shape, 6)
        G = np.full(shape, w, np.float32)
        ref, bnd = FB.map_grad_reference(x, y, G)
        want = orc.ssim_l1_backward(x, y, 0.0, float(np.float32(w)), LB.C1, LB.C2, dtype=np.float64)
        # the two differ in the window alone (float32 outer product against the separable float64 one): within NCONV's allowance
        LB.check(ref, want, bnd, what=f"{family} {shape}")
        got32 = orc.ssim_l1_backward(x, y, np.float32(0.0), np.float32(w), LB.C1, LB.C2, dtype=np.float32)
        LB.check(got32, ref, bnd, what=f"{family} {shape} float32")


def test_argument_errors_are_refused_before_any_device_call(hip_lib_built):
    """No device is needed: every call below returns GSR_E_INVALID from the validation at the top of its entry."""
    import _gsr
    lib, E = _gsr.lib, -1
    assert E == lib.gsr_set_option(b"no-such-option", 1)          # GSR_E_INVALID, as the other host-only tests read it
    p = 4096                                                       # a non-NULL pointer value; never dereferenced by a refused call
    C, H, W = 3, 8, 9
    assert lib.gsr_photometric_scratch_floats(C, 33, 65) == 2 * 3 * 2 * 3 and lib.gsr_photometric_scratch_floats(0, 8, 8) == 0

    def fwd(rgb=p, alpha=p, gt=p, mask=p, bg=p, C=C, H=H, W=W, sums=p, scratch=p, planes=(p, p, p)):
        return lib.gsr_photometric_forward(rgb, alpha, gt, mask, bg, C, H, W, LB.C1, LB.C2, sums, scratch, planes[0], planes[1], planes[2], None)

    def bwd(rgb=p, alpha=p, gt=p, mask=p, bg=p, C=C, H=H, W=W, weights=p, planes=(p, p, p), drgb=p, dalpha=p):
        return lib.gsr_photometric_backward(rgb, alpha, gt, mask, bg, C, H, W, weights, planes[0], planes[1], planes[2], drgb, dalpha, None)

    def mapb(img1=p, img2=p, planes=6, H=H, W=W, G=p, pl=(p, p, p), out=p):
        return lib.gsr_ssim_map_backward(img1, img2, planes, H, W, G, pl[0], pl[1], pl[2], out, None)

    bad = [fwd(C=0), fwd(H=0), fwd(W=-1), fwd(rgb=None), fwd(gt=None), fwd(sums=None), fwd(scratch=None),
           fwd(bg=None), fwd(alpha=None, bg=None), fwd(mask=None, bg=None),
           fwd(planes=(p, None, None)), fwd(planes=(p, p, None)), fwd(planes=(None, p, p)), fwd(planes=(None, None, p)),
           bwd(C=0), bwd(H=-3), bwd(W=0), bwd(rgb=None), bwd(gt=None), bwd(weights=None),
           bwd(planes=(None, p, p)), bwd(planes=(p, None, p)), bwd(planes=(p, p, None)),
           bwd(bg=None), bwd(alpha=None, bg=None, dalpha=None), bwd(mask=None, bg=None),
           bwd(alpha=None), bwd(alpha=None, mask=None, bg=None),
           mapb(planes=0), mapb(H=0), mapb(W=0), mapb(img1=None), mapb(img2=None), mapb(G=None), mapb(pl=(None, p, p)), mapb(pl=(p, None, p)),
           mapb(pl=(p, p, None)), mapb(out=None)]
    assert bad == [E] * len(bad), bad
    assert b"gsr_ssim_map_backward" in lib.gsr_last_error()
    assert bwd(alpha=None) == E and b"dL_dalpha" in lib.gsr_last_error()
