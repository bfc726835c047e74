"""Photometric losses of the reference's train loop on the HIP path (reference: utils/loss_utils.py).

Same names and call shapes as the reference module: `l1_loss`, `l2_loss`, `ssim`, `fast_ssim`, `FusedSSIMMap`
(utils/loss_utils.py:24-97), plus `photometric_loss`, the fused form of train.py:167-173
`(1 - lambda_dssim) * l1_loss + lambda_dssim * (1 - ssim)` that runs ONE forward and ONE backward kernel, also on the
composites of train.py:158-159 (`alpha=`, `gt_alpha_mask=`, `background=`), which the kernels form while they load.
All of them call libgsr_hip.so (gsr_ssim_l1_forward / _backward, gsr_photometric_forward / _backward,
gsr_ssim_map_backward, include/gsr_hip.h); there is no torch-conv fallback.  Only the reference's window (size 11,
sigma 1.5, zero padding 5) is implemented.
"""
import weakref

import torch
from torch.autograd.function import once_differentiable

from _gsr import check, check_sink_tensor, f32c, lib, ptr, require_cuda, require_entry, stream_ptr

require_entry(lib, "gsr_photometric_forward")       # the composited loss and the SSIM-map gradient

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def _chw(img, name):
    """The image as contiguous float32 planes [B*C, H, W]: the kernels treat every plane on its own, so a batch is more planes."""
    require_cuda(img, name)
    if img.dim() == 4:
        img = img.reshape(img.size(0) * img.size(1), img.size(2), img.size(3))
    if img.dim() != 3:
        raise ValueError(f"{name}: expected (C,H,W) or (B,C,H,W), got {tuple(img.shape)}")
    return f32c(img, name)


def _ssim_l1_forward(img1, img2, c1, c2, want_map, need_grad):
    """One gsr_ssim_l1_forward call on the images as planes: (x, y, sums, smap or None, maps or None), smap the per-pixel SSIM map
    [P,H,W] and maps the three derivative planes [3,P,H,W] that both backward entries take."""
    x, y = _chw(img1, "img1"), _chw(img2, "img2")
    if x.shape != y.shape:
        raise ValueError(f"image shapes differ: {tuple(x.shape)} vs {tuple(y.shape)}")
    P, H, W = x.shape
    dev = x.device
    sums = torch.empty(2, dtype=torch.float32, device=dev)
    smap = torch.empty((P, H, W), dtype=torch.float32, device=dev) if want_map else None
    maps = torch.empty((3, P, H, W), dtype=torch.float32, device=dev) if need_grad else None
    scratch = torch.empty(max(1, int(lib.gsr_ssim_l1_scratch_floats(P, H, W))), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.gsr_ssim_l1_forward(ptr(x), ptr(y), P, H, W, float(c1), float(c2), ptr(sums), ptr(scratch), ptr(smap),
                                      ptr(maps[0]) if need_grad else None, ptr(maps[1]) if need_grad else None,
                                      ptr(maps[2]) if need_grad else None, stream_ptr(dev)), "gsr_ssim_l1_forward")
    return x, y, sums, smap, maps


class _SsimL1(torch.autograd.Function):
    """sums = [sum |img1 - img2|, sum ssim_map]; gradient w.r.t. img1 only (the ground truth gets none, as in
    FusedSSIMMap.backward, utils/loss_utils.py:33-38)."""

    @staticmethod
    def forward(ctx, img1, img2, c1, c2, want_map):
        x, y, sums, smap, maps = _ssim_l1_forward(img1, img2, c1, c2, want_map, img1.requires_grad)
        ctx.save_for_backward(x, y, maps)
        # kept beside the saved tensors: l1_loss() and ssim() share this node (see _sums), and a caller who runs two backward passes —
        # l1.backward(retain_graph=True) for the render graph, then ssim.backward(), two graphs in the reference — reaches it twice, the
        # second time after autograd has released the saved tensors (x, y are inputs and maps an intermediate: no reference cycle)
        ctx.kept = (x, y, maps)
        ctx.versions = (x._version, y._version)
        ctx.ran = False
        ctx.in_shape = img1.shape
        ctx.want_map = want_map
        if want_map:
            ctx.mark_non_differentiable(smap)
            return sums, smap
        return sums, torch.empty(0, device=x.device)

    @staticmethod
    def backward(ctx, g_sums, _):
        global _last_sums
        last = _last_sums              # (read once: another host thread may replace or clear it between a test and a use)
        if last is not None and last[4].grad_fn is not None and getattr(last[4].grad_fn, "kept", None) is ctx.kept:
            _last_sums = None          # consumed: a later l1_loss / ssim call on the same tensors starts a fresh forward (and a fresh graph)
        if not ctx.ran:
            # first pass: autograd's own checks apply (an input modified in place since the forward raises here)
            x, y, maps = ctx.saved_tensors
            ctx.ran = True
        else:
            try:
                x, y, maps = ctx.saved_tensors  # a later pass with the buffers retained (retain_graph=True)
            except RuntimeError as ex:
                if "freed" not in str(ex):
                    raise
                x, y, maps = ctx.kept           # a later pass through the shared node after autograd released the buffers
                if (x._version, y._version) != ctx.versions:
                    raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace "
                                       "operation: an input of the fused SSIM + L1 loss changed after its forward") from ex
        C, H, W = x.shape
        grad = torch.empty_like(x)
        w = f32c(g_sums, "grad_sums")
        with torch.cuda.device(x.device):
            check(lib.gsr_ssim_l1_backward(ptr(x), ptr(y), C, H, W, ptr(w), ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(grad),
                                           stream_ptr(x.device)), "gsr_ssim_l1_backward")
        return grad.view(ctx.in_shape), None, None, None, None


_last_sums = None     # (weak image, its version, weak target, its version, weak result, grad mode) of the most recent _sums call


def _sums(img1, img2):
    """[sum |img1 - img2|, sum ssim_map].  The reference's loop calls l1_loss(image, gt) and then ssim(image, gt) on the same two
    tensors (train.py:167-173); both are read off ONE pair of sums, so the second call returns the first call's result (same tensor
    objects, unchanged since — version counters —, same grad mode) instead of running the fused forward, and later the fused backward,
    a second time.  The images are held weakly; the two-float result (and through its graph node the forward's saved planes, ~100 MB at
    1080p, and the render graph behind the image) is held until a backward pass consumes it, the next call replaces it or
    clear_cache() is called: the caller's `sums[0] / n` keeps the node alive, not the Python object.
    What the key cannot see: an image buffer refilled through its raw pointer (this library's own C-ABI writes, `.data` assignments) keeps
    object and version — call clear_cache() (or use photometric_loss, one explicit call) when reusing buffers that way."""
    global _last_sums
    last = _last_sums                  # (read once: another host thread may replace or clear it between the test and the unpacking)
    if last is not None:
        r1, v1, r2, v2, s, mode = last
        if r1() is img1 and r2() is img2 and img1._version == v1 and img2._version == v2 and mode == torch.is_grad_enabled():
            return s
    s = _SsimL1.apply(img1, img2, C1, C2, False)[0]
    _last_sums = (weakref.ref(img1), img1._version, weakref.ref(img2), img2._version, s, torch.is_grad_enabled())
    return s


def clear_cache():
    """Forget the result shared between l1_loss() and ssim() (see _sums)."""
    global _last_sums
    _last_sums = None


def l1_loss(network_output, gt):
    # utils/loss_utils.py:40-41
    return _sums(network_output, gt)[0] / network_output.numel()


def l2_loss(network_output, gt):
    # utils/loss_utils.py:43-44 (plain elementwise; not on the train-step path)
    return ((network_output - gt) ** 2).mean()


def ssim(img1, img2, window_size=11, size_average=True):
    # utils/loss_utils.py:62-97
    if window_size != 11:
        raise NotImplementedError("only the reference's 11x11 window is implemented on the HIP path")
    if not size_average:
        # the per-image mean `ssim_map.mean(1).mean(1).mean(1)` of a batch [B,C,H,W] (a [C,H,W] image counts as a batch of one)
        smap = FusedSSIMMap.apply(C1, C2, img1, img2)
        if smap.dim() == 3:
            smap = smap[None]
        return smap.mean(1).mean(1).mean(1)
    return _sums(img1, img2)[1] / img1.numel()


def fast_ssim(img1, img2):
    # utils/loss_utils.py:95-97
    return _sums(img1, img2)[1] / img1.numel()


class FusedSSIMMap(torch.autograd.Function):
    """utils/loss_utils.py:24-38: the per-pixel SSIM map of [C,H,W] or [B,C,H,W] images, differentiable w.r.t. img1 under any
    reduction of the map (gsr_ssim_map_backward takes the map's upstream gradient per pixel); img2 gets no gradient."""

    @staticmethod
    def forward(ctx, c1, c2, img1, img2):
        if img1.shape != img2.shape:      # (stricter than the planes' shapes: the map is returned in img1's shape)
            raise ValueError(f"image shapes differ: {tuple(img1.shape)} vs {tuple(img2.shape)}")
        need_grad = ctx.needs_input_grad[2]
        x, y, _, smap, maps = _ssim_l1_forward(img1, img2, c1, c2, True, need_grad)
        if need_grad:
            ctx.save_for_backward(x, y, maps)
        return smap.view(img1.shape)

    @staticmethod
    def backward(ctx, opt_grad):
        x, y, maps = ctx.saved_tensors
        P, H, W = x.shape
        if P == 0 or H == 0 or W == 0:
            return None, None, torch.zeros_like(opt_grad), None
        g = f32c(opt_grad, "grad_map")
        grad = torch.empty_like(x)
        with torch.cuda.device(x.device):
            check(lib.gsr_ssim_map_backward(ptr(x), ptr(y), P, H, W, ptr(g), ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(grad),
                                            stream_ptr(x.device)), "gsr_ssim_map_backward")
        return None, None, grad.view(opt_grad.shape), None


def _hw_plane(t, name, H, W, dev):
    """alpha / gt_alpha_mask as a float32 [H, W] plane on the image's device ([1, H, W] accepted; bool and uint8 masks converted)."""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.device != dev:
        raise ValueError(f"{name}: expected a tensor on {dev}, got {t.device if torch.is_tensor(t) else type(t).__name__}")
    if t.dim() == 3 and t.size(0) == 1:
        t = t[0]
    if tuple(t.shape) != (H, W):
        raise ValueError(f"{name}: expected ({H},{W}) or (1,{H},{W}), got {tuple(t.shape)}")
    if t.dtype in (torch.bool, torch.uint8):
        t = t.to(torch.float32)
    return t


class _CompositedSsimL1(torch.autograd.Function):
    """sums = [sum |v - g|, sum ssim_map(v, g)] of the composites v = image * alpha + (1 - alpha) * background and
    g = gt * mask + (1 - mask) * background (train.py:158-159), formed inside the kernels.  Gradients go to the image and to
    alpha, each only when it requires one; the ground truth, the mask and the background get none."""

    @staticmethod
    def forward(ctx, image, alpha, gt, mask, background):
        x, y = f32c(image, "image"), f32c(gt, "gt_image")
        a = None if alpha is None else f32c(alpha, "alpha")
        m = None if mask is None else f32c(mask, "gt_alpha_mask")
        C, H, W = x.shape[-3:]
        dev = x.device
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        maps = torch.empty((3, C, H, W), dtype=torch.float32, device=dev) if need_grad else None
        scratch = torch.empty(max(1, int(lib.gsr_photometric_scratch_floats(C, H, W))), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(lib.gsr_photometric_forward(ptr(x), ptr(a), ptr(y), ptr(m), ptr(background), C, H, W, C1, C2, ptr(sums), ptr(scratch),
                                              ptr(maps[0]) if need_grad else None, ptr(maps[1]) if need_grad else None,
                                              ptr(maps[2]) if need_grad else None, stream_ptr(dev)), "gsr_photometric_forward")
        ctx.save_for_backward(x, a, y, m, background, maps)
        ctx.shape = (C, H, W)
        return sums

    @staticmethod
    def backward(ctx, g_sums):
        x, a, y, m, background, maps = ctx.saved_tensors
        C, H, W = ctx.shape
        w = f32c(g_sums, "grad_sums")
        g_img = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        g_alpha = torch.empty_like(a) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(x.device):
            check(lib.gsr_photometric_backward(ptr(x), ptr(a), ptr(y), ptr(m), ptr(background), C, H, W, ptr(w), ptr(maps[0]), ptr(maps[1]),
                                               ptr(maps[2]), ptr(g_img), ptr(g_alpha), stream_ptr(x.device)), "gsr_photometric_backward")
        return g_img, g_alpha, None, None, None


def _composited_sums(image, gt_image, alpha, gt_alpha_mask, background):
    require_cuda(image, "image")
    require_cuda(gt_image, "gt_image")
    if image.dim() not in (3, 4) or (image.dim() == 4 and image.size(0) != 1):
        raise ValueError(f"image: expected (C,H,W) or (1,C,H,W) with alpha / gt_alpha_mask / background, got {tuple(image.shape)}")
    if image.shape != gt_image.shape:
        raise ValueError(f"image shapes differ: {tuple(image.shape)} vs {tuple(gt_image.shape)}")
    if background is None:
        raise ValueError("alpha or gt_alpha_mask given without a background")
    C, H, W = image.shape[-3:]
    if C == 0 or H == 0 or W == 0:
        raise ValueError(f"image: empty image {tuple(image.shape)}")
    dev = image.device
    a = _hw_plane(alpha, "alpha", H, W, dev)
    m = _hw_plane(gt_alpha_mask, "gt_alpha_mask", H, W, dev)
    if torch.is_tensor(background):
        if background.device != dev:
            raise ValueError(f"background: expected a tensor on {dev}, got {background.device}")
        bg = background.detach().to(torch.float32).reshape(-1).contiguous()
    else:
        bg = torch.tensor([float(b) for b in background], dtype=torch.float32, device=dev)
    if bg.numel() != C:
        raise ValueError(f"background: expected {C} values, got {bg.numel()}")
    return _CompositedSsimL1.apply(image, a, gt_image, m, bg)


def photometric_loss(image, gt_image, lambda_dssim=0.2, *, alpha=None, gt_alpha_mask=None, background=None):
    """train.py:167-173: (1 - lambda) * L1 + lambda * (1 - SSIM), one fused forward and one fused backward kernel.
    With alpha [H,W] / gt_alpha_mask [H,W] (or [1,H,W]) and background [C] it is the loss of train.py:156-159, 167-174 on
    image * alpha + (1 - alpha) * background and gt_image * mask + (1 - mask) * background, composited inside the same two kernels
    (alpha is not clamped, as there); the gradient reaches `image` and `alpha`.  That form makes one explicit call: it does not
    share its result with l1_loss() / ssim()."""
    if alpha is None and gt_alpha_mask is None and background is None:
        s = _sums(image, gt_image)
    else:
        s = _composited_sums(image, gt_image, alpha, gt_alpha_mask, background)
    n = image.numel()
    return (1.0 - lambda_dssim) * (s[0] / n) + lambda_dssim * (1.0 - s[1] / n)


class _NormalErrorSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rend_normal, surf_normal, mask):
        rn, sn = rend_normal.float().contiguous(), surf_normal.float().contiguous()
        if rn.dim() != 3 or rn.shape[0] != 3 or rn.shape != sn.shape:
            raise ValueError("normal_consistency_loss: expected two [3,H,W] tensors")
        H, W = rn.shape[1], rn.shape[2]
        mk = None
        if mask is not None:
            mk = mask.float().contiguous()
            if mk.numel() != H * W:
                raise ValueError("normal_consistency_loss: mask must have H*W elements")
        sums = torch.empty(2, dtype=torch.float32, device=rn.device)
        scratch = torch.empty(int(lib.gsr_normal_loss_scratch_floats()), dtype=torch.float32, device=rn.device)
        with torch.cuda.device(rn.device):
            check(lib.gsr_normal_loss_forward(ptr(rn), ptr(sn), ptr(mk), H, W, ptr(sums), ptr(scratch), stream_ptr(rn.device)), "gsr_normal_loss_forward")
        ctx.save_for_backward(rn, sn, mk) if mk is not None else ctx.save_for_backward(rn, sn)
        ctx.has_mask = mk is not None
        return sums[0]

    @staticmethod
    def backward(ctx, g_sum):
        saved = ctx.saved_tensors
        rn, sn = saved[0], saved[1]
        mk = saved[2] if ctx.has_mask else None
        g = g_sum.float().reshape(1).contiguous()
        g_rn, g_sn = torch.empty_like(rn), torch.empty_like(sn)
        with torch.cuda.device(rn.device):
            check(lib.gsr_normal_loss_backward(ptr(rn), ptr(sn), ptr(mk), rn.shape[1], rn.shape[2], ptr(g), ptr(g_rn), ptr(g_sn), stream_ptr(rn.device)),
                  "gsr_normal_loss_backward")
        return g_rn, g_sn, None


def normal_consistency_loss(rend_normal, surf_normal, lambda_normal=1.0, env_scope_mask=None):
    """train.py:182-189: lambda_normal * mean((1 - (rend_normal * surf_normal).sum(dim=0))[None] [* env_scope_mask]) as one fused
    kernel each way (extension; the reference spells it with five torch ops).  The mask receives no gradient (it is the
    rasterizer's binary env-scope plane, which has none in the reference's backward either)."""
    n = rend_normal.shape[1] * rend_normal.shape[2]
    return lambda_normal * (_NormalErrorSum.apply(rend_normal, surf_normal, env_scope_mask) / n)


# ------------------------------------------------------------------------------------------- env scope (opt.use_env_scope)
# train.py:56-63, 176-179 of the reference: the sphere test of every Gaussian centre and the reflection-mask loss over the centres outside
# it, on gsr_env_scope_forward / _backward (include/gsr_hip_scope.h): one pass over the points each way and no host read.
def _scope_sphere(center, radius):
    """(cx, cy, cz, radius2) as the Python floats the library takes by value; ctypes rounds them to float32 exactly as
    `torch.tensor(center)` and torch's comparison against the Python float `radius ** 2` do.  A tensor centre is read on the host
    (a device tensor costs a synchronisation: pass the numbers the options hold)."""
    c = [float(v) for v in (center.detach().reshape(-1).tolist() if torch.is_tensor(center) else center)]
    if len(c) != 3:
        raise ValueError(f"env scope: the centre must have three coordinates, got {len(c)}")
    return c[0], c[1], c[2], float(radius) ** 2


def _scope_xyz(xyz):
    require_cuda(xyz, "xyz")
    if xyz.dim() != 2 or xyz.size(1) != 3:
        raise ValueError(f"env scope: expected xyz of shape (P,3), got {tuple(xyz.shape)}")
    return xyz.detach().float().contiguous()


def _scope_forward(x, refl, sphere, want_inside=True):
    """One gsr_env_scope_forward call: (inside, outside, sums); sums is None without refl."""
    P, dev = x.size(0), x.device
    inside = torch.empty(P, dtype=torch.bool, device=dev) if want_inside else None
    outside = torch.empty(P, dtype=torch.bool, device=dev)
    sums = scratch = None
    if refl is not None:
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        scratch = torch.empty(int(lib.gsr_env_scope_scratch_floats()), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.gsr_env_scope_forward(P, ptr(x), ptr(refl), sphere[0], sphere[1], sphere[2], sphere[3], ptr(inside), ptr(outside), ptr(sums),
                                        ptr(scratch), stream_ptr(dev)), "gsr_env_scope_forward")
    return inside, outside, sums


def _scope_backward(outside, sums, g, grad, accumulate):
    """grad (+)= outside ? g / count : 0 (gsr_env_scope_backward); g is one float on the device."""
    P = outside.numel()
    if P == 0:
        return
    with torch.cuda.device(outside.device):
        check(lib.gsr_env_scope_backward(P, ptr(outside), ptr(sums), ptr(g), ptr(grad), 1 if accumulate else 0, stream_ptr(outside.device)),
              "gsr_env_scope_backward")


def env_scope_masks(xyz, center, radius):
    """(inside, outside): two torch.bool [P] tensors from one launch,
        inside  = ((xyz - center[None]) ** 2).sum(-1) < radius ** 2      (gaussian_renderer.render's env_scope_mask)
        outside = ((xyz - center[None]) ** 2).sum(-1) > radius ** 2      (train.py:61-63, get_outside_msk)
    with the float32 roundings of those expressions.  Neither is the other's negation: a centre exactly on the sphere or with a NaN
    coordinate is in neither.  `center`: three numbers (passed by value: no device copy) or a tensor."""
    require_entry(lib, "gsr_env_scope_forward")
    x = _scope_xyz(xyz)
    inside, outside, _ = _scope_forward(x, None, _scope_sphere(center, radius))
    return inside, outside


class _ReflScopeLoss(torch.autograd.Function):
    """loss = mean of refl over the outside points; gradient to refl only (the sphere test has none in the reference either)."""

    @staticmethod
    def forward(ctx, refl, xyz, sphere, grad_sink, accumulate):
        x = _scope_xyz(xyz)
        if refl.dim() not in (1, 2) or refl.numel() != x.size(0):
            raise ValueError(f"refl_scope_loss: expected refl of shape (P,) or (P,1) with P = {x.size(0)}, got {tuple(refl.shape)}")
        r = refl.detach().float().contiguous()
        if grad_sink is not None:
            check_sink_tensor("grad sink", "refl", grad_sink, refl.shape, r.device, aligned=False)
        inside, outside, sums = _scope_forward(x, r, sphere)
        ctx.save_for_backward(outside, sums)
        ctx.sink, ctx.accumulate, ctx.in_shape, ctx.in_dtype = grad_sink, bool(accumulate), refl.shape, refl.dtype
        ctx.mark_non_differentiable(inside, outside)
        return sums[0] / sums[1], inside, outside

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _gi, _go):
        outside, sums = ctx.saved_tensors
        g = g_loss.float().reshape(1).contiguous()
        if ctx.sink is not None:
            _scope_backward(outside, sums, g, ctx.sink, ctx.accumulate)
            return None, None, None, None, None
        grad = torch.empty(ctx.in_shape, dtype=torch.float32, device=outside.device)
        _scope_backward(outside, sums, g, grad, False)
        return grad.to(ctx.in_dtype), None, None, None, None


def refl_scope_loss(refl, xyz, center, radius, grad_sink=None, accumulate=False):
    """(loss, inside, outside) of the reference's env-scope branch (train.py:61-63, 176-179):
        loss = refl[outside].mean(),  outside = torch.sum((xyz - center[None]) ** 2, dim=-1) > radius ** 2
    as one fused pass each way: no nonzero, no host read.  `loss` is a 0-dim device tensor, sum / count formed on the device: NaN when no
    point is outside, as torch's mean of an empty selection (which, like here, then sends no gradient to any row).  `inside` and `outside`
    are the masks of env_scope_masks (non-differentiable).  The gradient reaches `refl` ([P] or [P,1], ACTIVATED strengths) only.
    grad_sink: a contiguous float32 tensor of refl's shape; the backward then writes (accumulate=False: every element, zeros where the
    point is not outside) or adds (accumulate=True: outside rows only) dL/drefl straight into it and autograd receives None for refl —
    the semantics of the rasterizer's sinks (_raster_api.GradSink)."""
    require_entry(lib, "gsr_env_scope_forward")
    if accumulate and grad_sink is None:
        raise ValueError("refl_scope_loss: accumulate=True needs a grad_sink to add to")
    require_cuda(refl, "refl")
    return _ReflScopeLoss.apply(refl, xyz, _scope_sphere(center, radius), grad_sink, accumulate)
