"""The composited photometric loss (csrc/gsr_loss.hip: gsr_photometric_forward / _backward) against the float64 oracle per
element, within the error bounds of tests/loss_front_bounds.py: every tile and halo offset, one to five channels, alpha and
mask each given or NULL, alpha planes with exact 0 / 1 regions across tile edges, ramps, noise and values outside [0, 1],
binary and soft masks, three backgrounds; a thin image; an alpha impulse at tile corners.  Bit-exact properties of the entry,
and the autograd wrapper utils.loss_utils.photometric_loss(alpha=, gt_alpha_mask=, background=)."""
import numpy as np
import pytest
import torch

import loss_bounds as LB
import loss_front_bounds as FB

pytestmark = pytest.mark.gpu
W_L1, W_SSIM = 0.8, -0.2
NAN = float("nan")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def gpu_front(case, w_l1=W_L1, w_ssim=W_SSIM, want_rgb=True, want_alpha=None):
    """C ABI forward and backward on a front_case; every output pre-filled with NaN, so that an element the kernels never write
    fails the comparison.  Returns float32 numpy outputs (sums as a [2] array)."""
    from _gsr import check, lib, stream_ptr
    rgb, gt, alpha, mask, bg = (_dev(case[k]) for k in ("rgb", "gt", "alpha", "mask", "bg"))
    if want_alpha is None:
        want_alpha = alpha is not None
    C, H, W = case["rgb"].shape
    n = int(lib.gsr_photometric_scratch_floats(C, H, W))
    assert n == 2 * C * ((H + 31) // 32) * ((W + 31) // 32)
    sums = torch.full((2,), NAN, device="cuda")
    scratch = torch.full((n,), NAN, device="cuda")
    planes = torch.full((3, C, H, W), NAN, device="cuda")
    s = stream_ptr(rgb.device)
    check(lib.gsr_photometric_forward(_p(rgb), _p(alpha), _p(gt), _p(mask), _p(bg), C, H, W, LB.C1, LB.C2, _p(sums), _p(scratch),
                                      _p(planes[0]), _p(planes[1]), _p(planes[2]), s), "gsr_photometric_forward")
    w = torch.tensor([w_l1, w_ssim], dtype=torch.float32, device="cuda")
    drgb = torch.full((C, H, W), NAN, device="cuda") if want_rgb else None
    dalpha = torch.full((H, W), NAN, device="cuda") if want_alpha else None
    check(lib.gsr_photometric_backward(_p(rgb), _p(alpha), _p(gt), _p(mask), _p(bg), C, H, W, _p(w), _p(planes[0]), _p(planes[1]),
                                       _p(planes[2]), _p(drgb), _p(dalpha), s), "gsr_photometric_backward")
    torch.cuda.synchronize()
    assert not torch.isnan(planes).any()
    out = dict(sums=sums.cpu().numpy(), drgb=None if drgb is None else drgb.cpu().numpy(), dalpha=None if dalpha is None else dalpha.cpu().numpy(),
               planes=planes.cpu().numpy())
    out["l1"], out["ssim"] = float(out["sums"][0]), float(out["sums"][1])
    return out


def check_case(case, what):
    ref, bnd = FB.front_reference(case, W_L1, W_SSIM)
    got = gpu_front(case)
    FB.check_front(got, ref, bnd, what)
    return got, ref, bnd


def _variety(i, family):
    bg = FB.BACKGROUNDS[i % 3]
    if family == "checker" and bg == FB.BACKGROUNDS[1]:
        # a render of exact ones on a white background is 1 * a + (1 - a) * 1 for every alpha: it ties with the background the mask
        # leaves, whatever the seed, and rounds for a < 0.5.  (On black the same composite is exact.)  White is left to the other families.
        bg = FB.BACKGROUNDS[2]
    return dict(combo=FB.COMBOS[i % 4], alpha_kind=FB.ALPHA_KINDS[(i + i // 4) % 4], mask_kind=FB.MASK_KINDS[(i // 2) % 2], background=bg)


@pytest.mark.parametrize("family", LB.FAMILIES)
def test_tile_and_halo_offsets(family):
    """H and W over the tile and halo offsets, C in {1, 2, 3, 5} (the backward's channel loop), all four combinations of alpha and
    mask given or NULL, every plane kind and background."""
    k = LB.FAMILIES.index(family)
    seen = set()
    for i, shape in enumerate(FB.front_shapes(k, 24)):
        kw = _variety(i + k, family)
        seen.add(kw["combo"])
        check_case(FB.front_case(family, shape, 200 + i, **kw), f"{family} {shape} {kw}")
    assert len(seen) == 4


@pytest.mark.parametrize("combo", FB.COMBOS)
def test_thin_image(combo):
    check_case(FB.front_case("uniform", (3, 513, 7), 7, combo, "outside", "soft"), f"thin {combo}")


def test_alpha_impulse_footprint():
    """rgb == gt and alpha == mask == 1 (v == g exactly: SSIM 1, zero gradient) except alpha at ONE pixel, a tile corner: both
    gradients match the reference inside the 21 x 21 box around it and are zero (within the bound) outside."""
    H, W = 75, 101
    base, _ = LB.loss_pair("lowpass", (3, H, W), 17)
    bg = np.array([0.0, 1.0, 0.5], np.float32)
    for (py, px) in [(31, 31), (32, 32), (0, 0), (H - 1, W - 1), (63, 32), (31, 64)]:
        alpha = np.ones((H, W), np.float32)
        alpha[py, px] = 0.5
        case = dict(rgb=base, gt=base.copy(), alpha=alpha, mask=np.ones((H, W), np.float32), bg=bg)
        got, ref, bnd = check_case(case, f"impulse {(py, px)}")
        box = np.zeros((H, W), bool)
        box[max(0, py - 10):py + 11, max(0, px - 10):px + 11] = True
        assert np.abs(ref["drgb"][:, ~box]).max() <= 1e-12 and np.abs(ref["dalpha"][~box]).max() <= 1e-12, (py, px)
        assert (np.abs(got["drgb"][:, ~box]) <= bnd["drgb"][:, ~box]).all(), (py, px)
        assert (np.abs(got["dalpha"][~box]) <= bnd["dalpha"][~box]).all(), (py, px)
        assert np.abs(got["drgb"][:, box]).max() > 1e-3 and np.abs(got["dalpha"][box]).max() > 1e-3, (py, px)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("shape", [(3, 43, 65), (5, 33, 31)])
def test_unit_planes_are_bitwise_the_call_without_planes(shape):
    """alpha == 1 and mask == 1 everywhere: compositing is exact, so sums and dL/drgb are bit for bit those of the NULL call."""
    C, H, W = shape
    plain = FB.front_case("hdr", shape, 3, (False, False))
    ones = dict(plain, alpha=np.ones((H, W), np.float32), mask=np.ones((H, W), np.float32))
    a, b = gpu_front(plain), gpu_front(ones)
    assert _same_bits(a["sums"], b["sums"]) and _same_bits(a["drgb"], b["drgb"])


def test_repeated_calls_and_optional_outputs_are_bitwise_identical():
    case = FB.front_case("uniform", (3, 65, 43), 5, (True, True), "outside", "soft")
    a, b = gpu_front(case), gpu_front(case)
    for k in ("sums", "drgb", "dalpha"):
        assert _same_bits(a[k], b[k]), k
    only_rgb = gpu_front(case, want_alpha=False)
    only_alpha = gpu_front(case, want_rgb=False)
    assert only_rgb["dalpha"] is None and _same_bits(only_rgb["drgb"], a["drgb"])
    assert only_alpha["drgb"] is None and _same_bits(only_alpha["dalpha"], a["dalpha"])


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 32, 32), (3, 33, 31), (3, 43, 65), (5, 33, 31)])
def test_call_without_planes_is_bitwise_the_training_loss(shape):
    """alpha, gt_mask and background NULL: the forward is the kernel gsr_ssim_l1_forward runs, so both sums and the three derivative
    planes are bit for bit that entry's (all padding; exactly one tile; one pixel into a second tile row; a halo that reaches a third
    tile; five channels).  The two backwards are different kernels: each, on its own planes, is held to the float64 bounds."""
    from _gsr import check, lib, stream_ptr
    C, H, W = shape
    case = FB.front_case("hdr", shape, 3, (False, False))
    ref, bnd = FB.front_reference(case, W_L1, W_SSIM)
    front = gpu_front(case)
    x, y = _dev(case["rgb"]), _dev(case["gt"])
    sums = torch.full((2,), NAN, device="cuda")
    scratch = torch.full((int(lib.gsr_ssim_l1_scratch_floats(C, H, W)),), NAN, device="cuda")
    planes = torch.full((3, C, H, W), NAN, device="cuda")
    grad = torch.full((C, H, W), NAN, device="cuda")
    w = torch.tensor([W_L1, W_SSIM], dtype=torch.float32, device="cuda")
    s = stream_ptr(x.device)
    check(lib.gsr_ssim_l1_forward(_p(x), _p(y), C, H, W, LB.C1, LB.C2, _p(sums), _p(scratch), None, _p(planes[0]), _p(planes[1]), _p(planes[2]), s),
          "gsr_ssim_l1_forward")
    check(lib.gsr_ssim_l1_backward(_p(x), _p(y), C, H, W, _p(w), _p(planes[0]), _p(planes[1]), _p(planes[2]), _p(grad), s), "gsr_ssim_l1_backward")
    torch.cuda.synchronize()
    train = dict(sums=sums.cpu().numpy(), planes=planes.cpu().numpy(), drgb=grad.cpu().numpy())
    assert _same_bits(front["sums"], train["sums"]) and _same_bits(front["planes"], train["planes"])
    train["l1"], train["ssim"] = float(train["sums"][0]), float(train["sums"][1])
    FB.check_front(front, ref, bnd, f"photometric {shape}")
    FB.check_front(train, ref, bnd, f"ssim_l1 {shape}")


# ----------------------------------------------------------------------------------------------------- autograd wrapper
SHAPE = (3, 43, 65)
LAM = 0.2


@pytest.fixture(scope="module")
def py_case():
    case = FB.front_case("uniform", SHAPE, 31, (True, True), "outside", "soft")
    n = case["rgb"].size
    ref, bnd = FB.front_reference(case, (1.0 - LAM) / n, -LAM / n)
    ref1, bnd1 = FB.front_reference(case, 1.0, 1.0)          # (for the sums: they do not depend on the weights)
    return case, ref, bnd, ref1, bnd1


def test_photometric_loss_with_planes(py_case):
    from utils.loss_utils import photometric_loss
    case, ref, bnd, ref1, bnd1 = py_case
    n = case["rgb"].size
    image = _dev(case["rgb"]).requires_grad_(True)
    alpha = _dev(case["alpha"])[None].requires_grad_(True)          # [1, H, W], as the rasterizer's alpha plane
    loss = photometric_loss(image, _dev(case["gt"]), LAM, alpha=alpha, gt_alpha_mask=_dev(case["mask"])[None], background=_dev(case["bg"]))
    want = (1.0 - LAM) * ref1["l1"] / n + LAM * (1.0 - ref1["ssim"] / n)
    # the two sums' bounds, scaled, and the six float32 operations of the combination on values of at most 1
    allow = (1.0 - LAM) * bnd1["l1"] / n + LAM * bnd1["ssim"] / n + 6 * LB.U
    assert abs(loss.item() - want) <= allow
    loss.backward()
    assert image.grad.shape == SHAPE and alpha.grad.shape == (1,) + SHAPE[1:]
    LB.check(image.grad.cpu().numpy(), ref["drgb"], bnd["drgb"], what="image.grad")
    LB.check(alpha.grad[0].cpu().numpy(), ref["dalpha"], bnd["dalpha"], what="alpha.grad")


def test_photometric_loss_without_alpha_gradient_and_with_a_bool_mask(py_case):
    from utils.loss_utils import photometric_loss
    case, ref, bnd, _, _ = py_case
    image = _dev(case["rgb"]).requires_grad_(True)
    alpha = _dev(case["alpha"])
    photometric_loss(image, _dev(case["gt"]), LAM, alpha=alpha, gt_alpha_mask=_dev(case["mask"]), background=tuple(float(b) for b in case["bg"])).backward()
    assert alpha.grad is None
    LB.check(image.grad.cpu().numpy(), ref["drgb"], bnd["drgb"], what="image.grad")
    # alpha alone requires a gradient; the (1, C, H, W) call shape
    alpha = _dev(case["alpha"]).requires_grad_(True)
    photometric_loss(_dev(case["rgb"])[None], _dev(case["gt"])[None], LAM, alpha=alpha, gt_alpha_mask=_dev(case["mask"]), background=_dev(case["bg"])).backward()
    LB.check(alpha.grad.cpu().numpy(), ref["dalpha"], bnd["dalpha"], what="alpha.grad")
    # a bool (or uint8) mask is the float mask
    binary = FB.mask_plane("binary", SHAPE[1], SHAPE[2], 31)
    args = (_dev(case["rgb"]), _dev(case["gt"]), LAM)
    with torch.no_grad():
        f = photometric_loss(*args, gt_alpha_mask=_dev(binary), background=_dev(case["bg"]))
        b = photometric_loss(*args, gt_alpha_mask=_dev(binary) > 0.5, background=_dev(case["bg"]))
        u = photometric_loss(*args, gt_alpha_mask=(_dev(binary) > 0.5).to(torch.uint8), background=_dev(case["bg"]))
        plain = photometric_loss(*args)
    assert f.item() == b.item() == u.item() and f.item() != plain.item()


def test_photometric_loss_refuses_wrong_arguments(py_case):
    from utils.loss_utils import photometric_loss
    case = py_case[0]
    C, H, W = SHAPE
    image, gt, alpha, mask, bg = (_dev(case[k]) for k in ("rgb", "gt", "alpha", "mask", "bg"))
    for kw in (dict(alpha=alpha), dict(gt_alpha_mask=mask), dict(alpha=alpha, gt_alpha_mask=mask),      # a plane without a background
               dict(alpha=alpha[:, :-1], background=bg), dict(gt_alpha_mask=mask[None, None], background=bg),
               dict(alpha=alpha.expand(3, H, W), background=bg), dict(alpha=alpha.cpu(), background=bg),
               dict(gt_alpha_mask=mask.cpu(), background=bg), dict(alpha=alpha, background=bg[:2]), dict(alpha=alpha, background=bg.cpu()),
               dict(alpha=alpha, background=(0.0, 0.0))):
        with pytest.raises(ValueError):
            photometric_loss(image, gt, LAM, **kw)
    with pytest.raises(ValueError):
        photometric_loss(image, gt[:, :-1], LAM, alpha=alpha, background=bg)
    with pytest.raises(ValueError):
        photometric_loss(torch.stack([image, image]), torch.stack([gt, gt]), LAM, alpha=alpha, background=bg)
