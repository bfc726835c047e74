"""The per-pixel gradient of the SSIM map (csrc/gsr_loss.hip: gsr_ssim_map_backward) against its float64 reference within
the bounds of tests/loss_front_bounds.py, and what utils/loss_utils.py builds on it: FusedSSIMMap.backward under a masked
mean, ssim(size_average=False), batches, and the fused_ssim package."""
import numpy as np
import pytest
import torch

import loss_bounds as LB
import loss_front_bounds as FB

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_map_backward(x, y, G=None, weights=None):
    """Forward (derivative planes of gsr_ssim_l1_forward on P = x.shape[0] planes), then gsr_ssim_map_backward with G, or
    gsr_ssim_l1_backward with `weights`; the output pre-filled with NaN."""
    from _gsr import check, lib, stream_ptr
    X, Y = _dev(x), _dev(y)
    P, H, W = x.shape
    sums = torch.empty(2, device="cuda")
    scratch = torch.empty(max(1, int(lib.gsr_ssim_l1_scratch_floats(P, H, W))), device="cuda")
    planes = torch.full((3, P, H, W), NAN, device="cuda")
    s = stream_ptr(X.device)
    check(lib.gsr_ssim_l1_forward(X.data_ptr(), Y.data_ptr(), P, H, W, LB.C1, LB.C2, sums.data_ptr(), scratch.data_ptr(), None,
                                  planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), s), "gsr_ssim_l1_forward")
    out = torch.full_like(X, NAN)
    if G is not None:
        Gd = _dev(G)
        check(lib.gsr_ssim_map_backward(X.data_ptr(), Y.data_ptr(), P, H, W, Gd.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(),
                                        planes[2].data_ptr(), out.data_ptr(), s), "gsr_ssim_map_backward")
    else:
        w = torch.tensor(weights, dtype=torch.float32, device="cuda")
        check(lib.gsr_ssim_l1_backward(X.data_ptr(), Y.data_ptr(), P, H, W, w.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(),
                                       planes[2].data_ptr(), out.data_ptr(), s), "gsr_ssim_l1_backward")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("family", ["uniform", "lowpass", "bright_flat", "hdr", "steps", "identical"])
def test_random_sign_upstream_gradient(family):
    k = LB.FAMILIES.index(family)
    for i, shape in enumerate(FB.front_shapes(40 + k, 13)):
        x, y = LB.loss_pair(family, shape, 300 + i)
        G = np.random.RandomState(i).randn(*shape).astype(np.float32)
        ref, bnd = FB.map_grad_reference(x, y, G)
        LB.check(gpu_map_backward(x, y, G), ref, bnd, what=f"{family} {shape}")


def test_upstream_gradient_confined_to_one_tile():
    """G is zero outside the tile (1, 1): the gradient is zero (within the bound) beyond 5 pixels of it, which pins the halo of the
    staged products."""
    shape = (2, 75, 101)
    x, y = LB.loss_pair("uniform", shape, 9)
    G = np.zeros(shape, np.float32)
    G[:, 32:64, 32:64] = np.random.RandomState(9).randn(2, 32, 32)
    ref, bnd = FB.map_grad_reference(x, y, G)
    got = gpu_map_backward(x, y, G)
    LB.check(got, ref, bnd, what="one tile")
    reach = np.zeros(shape[1:], bool)
    reach[27:69, 27:69] = True
    assert np.abs(ref[:, ~reach]).max() == 0 and np.abs(got[:, ~reach]).max() == 0
    assert np.abs(got[:, 27, 27:69]).max() > 0 and np.abs(got[:, 27:69, 68]).max() > 0


@pytest.mark.parametrize("shape", [(3, 37, 65), (1, 64, 33), (5, 6, 11)])
def test_constant_upstream_gradient_is_the_sum_backward(shape):
    """G == w everywhere against gsr_ssim_l1_backward with weights {0, w}: each within its own bound of the same float64 value,
    so within the sum of the two of each other."""
    w = 0.37
    x, y = LB.loss_pair("uniform", shape, 12)
    ref, bnd = FB.map_grad_reference(x, y, np.full(shape, w, np.float32))
    ref0, bnd0 = LB.ssim_reference(x, y, 0.0, w)
    got = gpu_map_backward(x, y, np.full(shape, w, np.float32))
    got0 = gpu_map_backward(x, y, weights=[0.0, w])
    LB.check(got, ref, bnd, what="map backward")
    LB.check(got, got0, bnd + bnd0["grad"], what="map backward against the sum backward")


# ------------------------------------------------------------------------------------------------------ Python surface
B, C, H, W = 2, 3, 37, 65


@pytest.fixture(scope="module")
def batch():
    pairs = [LB.loss_pair("uniform", (C, H, W), 50 + b) for b in range(B)]
    x, y = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ref, bnd = LB.ssim_reference(x.reshape(B * C, H, W), y.reshape(B * C, H, W), 0.0, 1.0)
    return x, y, ref["map"].reshape(B, C, H, W), bnd["map"].reshape(B, C, H, W)


def _mean_bound(b_map, ref_map):
    """A float32 mean of the map: the elements' own bounds, and torch's reduction (a thread adds at most a few dozen elements
    in sequence before the tree; 64 roundings of the mean magnitude is beyond any arrangement at these sizes)."""
    return b_map.mean() + 64 * LB.U * np.abs(ref_map).mean()


def test_fused_ssim_map_backward_under_a_masked_mean(batch):
    from utils.loss_utils import C1, C2, FusedSSIMMap
    x, y, ref_map, b_map = batch
    img1, img2 = _dev(x).requires_grad_(True), _dev(y)
    mask = _dev((np.random.RandomState(1).rand(B, 1, H, W) < 0.4).astype(np.float32))
    smap = FusedSSIMMap.apply(C1, C2, img1, img2)
    assert smap.shape == (B, C, H, W)
    LB.check(smap.detach().cpu().numpy(), ref_map, b_map, what="map")
    smap.retain_grad()
    ((smap * mask).sum() / (mask.sum() * C)).backward()
    G = smap.grad.cpu().numpy()                          # the upstream gradient the node received, bit for bit
    assert (G[mask.expand(B, C, H, W).cpu().numpy() == 0] == 0).all() and (G != 0).any()
    ref, bnd = FB.map_grad_reference(x.reshape(B * C, H, W), y.reshape(B * C, H, W), G.reshape(B * C, H, W))
    assert img1.grad.shape == (B, C, H, W)
    LB.check(img1.grad.cpu().numpy().reshape(B * C, H, W), ref, bnd, what="img1.grad")
    # the ground truth gets no gradient, and without a gradient to compute nothing is saved
    assert img2.grad is None
    assert FusedSSIMMap.apply(C1, C2, _dev(x), img2).grad_fn is None


def test_ssim_per_image(batch):
    from utils.loss_utils import ssim
    x, y, ref_map, b_map = batch
    img1, img2 = _dev(x).requires_grad_(True), _dev(y)
    per = ssim(img1, img2, size_average=False)
    assert per.shape == (B,)
    for b in range(B):
        assert abs(per[b].item() - ref_map[b].mean()) <= _mean_bound(b_map[b], ref_map[b]), b
    (per * torch.tensor([1.0, -2.0], device="cuda")).sum().backward()
    d = torch.zeros(B, C, H, W, device="cuda", requires_grad=True)          # the same reduction's upstream gradient, bit for bit
    (d.mean(1).mean(1).mean(1) * torch.tensor([1.0, -2.0], device="cuda")).sum().backward()
    ref, bnd = FB.map_grad_reference(x.reshape(B * C, H, W), y.reshape(B * C, H, W), d.grad.cpu().numpy().reshape(B * C, H, W))
    LB.check(img1.grad.cpu().numpy().reshape(B * C, H, W), ref, bnd, what="img1.grad")
    # the batch on the sum path: (B, C) flattened into planes
    with torch.no_grad():
        mean = ssim(_dev(x), img2)
    assert abs(mean.item() - ref_map.mean()) <= _mean_bound(b_map, ref_map)
    with pytest.raises(NotImplementedError):
        ssim(img1, img2, window_size=7)


def test_fused_ssim_package(batch):
    from fused_ssim import fused_ssim
    from utils.loss_utils import clear_cache, ssim
    x, y, ref_map, b_map = batch
    x1, y1 = x[:1], y[:1]
    clear_cache()
    img1, img2 = _dev(x1).requires_grad_(True), _dev(y1)
    same = fused_ssim(img1, img2)
    plain = ssim(img1, img2)
    allow = _mean_bound(b_map[0], ref_map[0])
    assert abs(same.item() - ref_map[0].mean()) <= allow and abs(plain.item() - ref_map[0].mean()) <= allow
    with torch.no_grad():
        assert fused_ssim(img1, img2, train=False).item() == same.item()
    assert fused_ssim(img1, img2, train=False).grad_fn is None
    valid = fused_ssim(img1, img2, padding="valid")
    inner = (slice(None), slice(5, H - 5), slice(5, W - 5))
    assert abs(valid.item() - ref_map[0][inner].mean()) <= _mean_bound(b_map[0][inner], ref_map[0][inner])
    with pytest.raises(AssertionError):
        fused_ssim(img1, img2, padding="reflect")
    clear_cache()


def test_fused_ssim_valid_takes_no_gradient_from_border_map_pixels():
    """img2 = img1 except one pixel at (2, 2): the map moves at the pixels within 5 of it, of which "valid" keeps only rows and
    columns 5 .. 7.  The gradient is the reference's with the border of the upstream gradient zero, and differs from the
    "same" one (rescaled by the pixel counts) by far more than the bound."""
    from fused_ssim import fused_ssim
    Hh, Ww = 37, 43
    base, _ = LB.loss_pair("lowpass", (3, Hh, Ww), 21)
    x, y = base, base.copy()
    y[:, 2, 2] += 0.5
    grads = {}
    for padding in ("same", "valid"):
        img1 = _dev(x[None]).requires_grad_(True)
        fused_ssim(img1, _dev(y[None]), padding=padding).backward()
        grads[padding] = img1.grad[0].cpu().numpy()
    G = np.zeros((3, Hh, Ww), np.float32)
    d = torch.zeros(1, 3, Hh, Ww, device="cuda", requires_grad=True)
    d[:, :, 5:-5, 5:-5].mean().backward()
    G[:] = d.grad[0].cpu().numpy()
    assert (G[:, :5] == 0).all() and (G[:, :, :5] == 0).all() and (G[:, -5:] == 0).all() and (G[:, :, -5:] == 0).all() and G[0, 5, 5] > 0
    ref, bnd = FB.map_grad_reference(x, y, G)
    LB.check(grads["valid"], ref, bnd, what="valid")
    scale = (Hh * Ww) / ((Hh - 10) * (Ww - 10))
    assert np.abs(grads["same"][:, 0, 0] * scale - ref[:, 0, 0]).min() > 100 * bnd[:, 0, 0].max()
