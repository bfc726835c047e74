"""Fused SSIM + L1 (csrc/gsr_loss.hip) against the float64 oracle per element, within the error bounds of
tests/loss_bounds.py, at the shapes and contents where a 32 x 32 tile with a 42 x 42 halo goes wrong: every tile and halo
offset, thin images, full size, cancelling bright flat regions, HDR values, exact ties, impulses at tile edges.  Also the
autograd wrapper (utils/loss_utils.py): in-place changes between forward and backward raise, supported call sequences keep
the reference gradient."""
import numpy as np
import pytest
import torch

import loss_bounds as LB

pytestmark = pytest.mark.gpu
W_L1, W_SSIM = 0.8, -0.2


def gpu_loss(x, y, w_l1=W_L1, w_ssim=W_SSIM):
    """C ABI forward (sums, map, derivative planes) and backward on float32 [C, H, W]; outputs pre-filled with NaN so that an
    element the kernels never write fails the comparison."""
    from _gsr import check, lib, stream_ptr
    X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    C, H, W = x.shape
    sums = torch.full((2,), float("nan"), device="cuda")
    scratch = torch.empty(max(1, int(lib.gsr_ssim_l1_scratch_floats(C, H, W))), device="cuda")
    smap = torch.full_like(X, float("nan"))
    planes = torch.full((3, C, H, W), float("nan"), device="cuda")
    s = stream_ptr(X.device)
    check(lib.gsr_ssim_l1_forward(X.data_ptr(), Y.data_ptr(), C, H, W, LB.C1, LB.C2, sums.data_ptr(), scratch.data_ptr(), smap.data_ptr(),
                                  planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), s), "gsr_ssim_l1_forward")
    w = torch.tensor([w_l1, w_ssim], dtype=torch.float32, device="cuda")
    grad = torch.full_like(X, float("nan"))
    check(lib.gsr_ssim_l1_backward(X.data_ptr(), Y.data_ptr(), C, H, W, w.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(),
                                   planes[2].data_ptr(), grad.data_ptr(), s), "gsr_ssim_l1_backward")
    torch.cuda.synchronize()
    sums = sums.cpu().numpy()
    return dict(l1=float(sums[0]), ssim=float(sums[1]), map=smap.cpu().numpy(), grad=grad.cpu().numpy())


def check_loss(x, y, what):
    ref, bnd = LB.ssim_reference(x, y, W_L1, W_SSIM)
    got = gpu_loss(x, y)
    for k in ("l1", "ssim", "map", "grad"):
        LB.check(got[k], ref[k], bnd[k], what=f"{what} {k}")
    return got, ref, bnd


@pytest.mark.parametrize("family", LB.FAMILIES)
def test_tile_and_halo_offsets(family):
    """H and W over every tile / halo offset, C in {1, 2, 3, 5}."""
    for i, shape in enumerate(LB.ssim_shapes(LB.FAMILIES.index(family), 24)):
        x, y = LB.loss_pair(family, shape, 100 + i)
        got, ref, bnd = check_loss(x, y, f"{family} {shape}")
        if family == "ties":
            tied = x == y          # sign(0) = 0: the gradient there is the SSIM term alone, which the bound already pins
            assert tied.any()
        if family == "constant_pair":
            # interior pixels (the window inside the image) have the closed-form SSIM of two constants; with the float32
            # window's sum s (1 - s ~ 1e-7) the variances are s (1 - s) a^2, not 0, which moves the map by ~1e-5
            a, b = float(np.float32(0.3)), float(np.float32(0.7))
            C, H, W = shape
            g = LB.window1d().astype(np.float32)
            s = float(np.outer(g, g).astype(np.float32).astype(np.float64).sum())
            closed = ((2 * s * s * a * b + LB.C1) * (2 * s * (1 - s) * a * b + LB.C2)
                      / ((s * s * (a * a + b * b) + LB.C1) * (s * (1 - s) * (a * a + b * b) + LB.C2)))
            inner = ref["map"][:, 5:H - 5, 5:W - 5]    # (the kernel's values there are held to the bound by check_loss)
            if inner.size:
                assert np.abs(inner - closed).max() <= 1e-9


@pytest.mark.parametrize("family", ["uniform", "steps"])
@pytest.mark.parametrize("shape", [(3, 2049, 7), (1, 7, 2049)])
def test_thin_images(family, shape):
    x, y = LB.loss_pair(family, shape, 7)
    check_loss(x, y, f"{family} {shape}")


@pytest.mark.parametrize("family", ["uniform", "bright_flat", "ties", "hdr"])
def test_full_size(family):
    x, y = LB.loss_pair(family, (3, 1080, 1920), 11)
    check_loss(x, y, family)


def test_4k():
    x, y = LB.loss_pair("lowpass", (3, 2160, 3840), 13)
    check_loss(x, y, "4k")


def test_impulse_footprint():
    """img2 = img1 except one pixel per channel, placed at every step offset of the tile and at the four corners: the gradient
    matches the reference inside the 21 x 21 neighbourhood and is zero (within the bound) outside it, which pins the halo
    indexing of the backward."""
    H, W = 75, 101
    pos = [(32 + o, 32 + (o + 5) % 32) for o in LB.STEP_OFFSETS] + [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (64 + 4, 64 + 31)]
    pos = [(min(py, H - 1), min(px, W - 1)) for py, px in pos]
    C = len(pos)
    base, _ = LB.loss_pair("lowpass", (1, H, W), 17)
    x = np.ascontiguousarray(np.repeat(base, C, 0))
    y = x.copy()
    for c, (py, px) in enumerate(pos):
        y[c, py, px] += 0.5
    got, ref, bnd = check_loss(x, y, "impulse")
    for c, (py, px) in enumerate(pos):
        box = np.zeros((H, W), bool)
        box[max(0, py - 10):py + 11, max(0, px - 10):px + 11] = True
        # the footprint itself: the reference vanishes outside the box, the kernel's gradient there is zero within the bound
        assert np.abs(ref["grad"][c][~box]).max() <= 1e-12, (py, px)
        assert (np.abs(got["grad"][c][~box]) <= bnd["grad"][c][~box]).all(), (py, px)
        assert np.abs(got["grad"][c][box]).max() > 1e-3, (py, px)


def test_batched_call_shape():
    """The (1, C, H, W) call shape of the reference's train loop, through the autograd wrapper."""
    from utils.loss_utils import _SsimL1, C1, C2
    x, y = LB.loss_pair("uniform", (3, 43, 65), 19)
    ref, bnd = LB.ssim_reference(x, y, W_L1, W_SSIM)
    a = torch.from_numpy(x)[None].cuda().requires_grad_(True)
    b = torch.from_numpy(y)[None].cuda()
    sums, smap = _SsimL1.apply(a, b, C1, C2, True)
    (sums * torch.tensor([W_L1, W_SSIM], device="cuda")).sum().backward()
    assert a.grad.shape == (1, 3, 43, 65)
    LB.check(smap.detach().cpu().numpy(), ref["map"], bnd["map"], what="map")
    LB.check(a.grad[0].cpu().numpy(), ref["grad"], bnd["grad"], what="grad")
    LB.check(float(sums[0].detach()), ref["l1"], bnd["l1"], what="l1")
    LB.check(float(sums[1].detach()), ref["ssim"], bnd["ssim"], what="ssim")


# ----------------------------------------------------------------------------------------------------- autograd wrapper
def _pair(seed=23, shape=(3, 40, 56)):
    x, y = LB.loss_pair("uniform", shape, seed)
    return x, y


def _reference_grad(x, y, w_l1, w_ssim):
    ref, bnd = LB.ssim_reference(x, y, w_l1, w_ssim)
    return ref["grad"], bnd["grad"]


@pytest.mark.parametrize("which", ["image", "gt"])
@pytest.mark.parametrize("form", ["photometric", "l1_plus_ssim"])
def test_in_place_change_between_forward_and_backward_raises(which, form):
    """As the reference's torch ops do: the backward must not mix the new pixels with the forward's SSIM planes."""
    from utils.loss_utils import clear_cache, l1_loss, photometric_loss, ssim
    clear_cache()
    x, y = _pair()
    leaf = torch.from_numpy(x).cuda().requires_grad_(True)
    image = leaf * 1.0                      # a non-leaf, like the render
    gt = torch.from_numpy(y).cuda()
    if form == "photometric":
        loss = photometric_loss(image, gt, 0.2)
    else:
        loss = 0.8 * l1_loss(image, gt) + 0.2 * (1.0 - ssim(image, gt))
    with torch.no_grad():
        (image if which == "image" else gt).add_(0.25)
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()
    clear_cache()


def test_supported_sequences_keep_the_reference_gradient():
    from utils.loss_utils import clear_cache, l1_loss, photometric_loss, ssim
    x, y = _pair(29)
    n = x.size
    gt = torch.from_numpy(y).cuda()
    ref, bnd = _reference_grad(x, y, 0.8 / n, -0.2 / n)

    def fresh():
        clear_cache()
        return torch.from_numpy(x).cuda().requires_grad_(True)
    a = fresh()
    photometric_loss(a, gt, 0.2).backward()
    LB.check(a.grad.cpu().numpy(), ref, bnd, what="photometric_loss")
    a = fresh()
    (0.8 * l1_loss(a, gt) + 0.2 * (1.0 - ssim(a, gt))).backward()
    LB.check(a.grad.cpu().numpy(), ref, bnd, what="0.8 l1 + 0.2 (1 - ssim)")
    # two passes through the one shared node: first with the buffers retained, then after autograd has released them
    r_l1, b_l1 = _reference_grad(x, y, 1.0 / n, 0.0)
    r_ss, b_ss = _reference_grad(x, y, 0.0, 1.0 / n)
    for retain in (True, False):
        a = fresh()
        l1, s = l1_loss(a, gt), ssim(a, gt)
        l1.backward(retain_graph=retain)
        LB.check(a.grad.cpu().numpy(), r_l1, b_l1, what=f"l1 pass, retain={retain}")
        a.grad = None
        s.backward()
        LB.check(a.grad.cpu().numpy(), r_ss, b_ss, what=f"ssim pass, retain={retain}")
    # a second pass after the release still refuses inputs changed in place since the forward
    a = fresh()
    g2 = gt.clone()
    l1, s = l1_loss(a, g2), ssim(a, g2)
    l1.backward()
    g2.add_(0.25)
    with pytest.raises(RuntimeError, match="inplace"):
        s.backward()
    clear_cache()
