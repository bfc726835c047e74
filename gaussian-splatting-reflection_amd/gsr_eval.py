"""Evaluation on the device: what the reference does after training to judge a model (render.py presents and saves every test
view, metrics.py scores the saved PNGs, eval_mae.py the normals), without leaving the GPU between the render and the number.

`MetricsTable` is a [views, 4] float64 table in device memory.  Every call of its `image()` / `normals()` fills one row with one
fused kernel (csrc/gsr_metrics.hip: gsr_image_metrics presents both images while it stages them, gsr_normal_mae is one pass over the
normals) and returns nothing; `result()` reads the whole table back once.  `evaluate_views` is render.py + metrics.py for a list of
views.  All native code; there is no torch fallback.

LPIPS (the third number metrics.py writes) is not provided: it needs the weights of a pretrained VGG network, which are not part of
this project.  Save the presented images (`keep_images=True` returns them as uint8) and run lpipsPyTorch on them where those weights
are available.
"""
import math

import numpy as np
import torch

from _gsr import GSR_PRESENT_CLAMP, GSR_PRESENT_QUANT8, check, f32c, lib, ptr, require_cuda, require_entry, stream_ptr

require_entry(lib, "gsr_image_metrics")       # the evaluation metrics (gsr_normal_mae comes with it)


def _plane(t, name, H, W):
    if t is None:
        return None
    require_cuda(t, name)
    if t.numel() != H * W:
        raise ValueError(f"{name}: expected H*W = {H * W} elements, got {tuple(t.shape)}")
    return f32c(t, name)


class MetricsTable:
    """[V, 4] float64 rows in device memory, one per view.  image() leaves {sum (v - g)^2, sum |v - g|, sum ssim_map, C*H*W} of the
    presented images, normals() {sum of the angular error in degrees over valid pixels, valid pixels, invalid pixels, H*W}.  Rows that
    were never written hold NaN.  Calls run on the current stream and never synchronise; result() does the one read-back."""

    def __init__(self, V, device="cuda"):
        self.device = torch.device(device)
        self.rows = torch.full((int(V), 4), float("nan"), dtype=torch.float64, device=self.device)
        self._scratch = None

    def _scratch_for(self, floats):
        # one scratch buffer for the table: calls on one stream run in order, and each call's second kernel has consumed it
        if self._scratch is None or self._scratch.numel() < floats:
            self._scratch = torch.empty(max(4, int(floats)), dtype=torch.float32, device=self.device)
        return self._scratch

    def _on_device(self, **tensors):
        """Every tensor handed to a kernel lives on the table's device: the kernel runs there and reads raw pointers."""
        for name, t in tensors.items():
            if t is not None and (not t.is_cuda or t.device != self.rows.device):
                raise ValueError(f"{name}: expected a tensor on {self.rows.device}, the table's device, got {t.device}")

    def _row(self, v):
        if not 0 <= v < self.rows.shape[0]:
            raise IndexError(f"row {v} of a table of {self.rows.shape[0]}")
        return self.rows.data_ptr() + 32 * v

    def image(self, v, img, gt, clamp=False, alpha=None, gt_mask=None, background=None, quantize8=False, img_u8=None, gt_u8=None):
        """Row v <- the three sums of img against gt ([C,H,W] float32), presented as render.py:48-62 does: clamp the render to [0, 1];
        composite the render with clamp(alpha) and the ground truth with gt_mask ([H,W] or [1,H,W], either may be None) onto
        background [C]; quantise both to 8 bits as save_image does.  img_u8 / gt_u8: uint8 [C,H,W] tensors that receive the
        presented images (quantize8 only)."""
        require_cuda(img, "img")
        require_cuda(gt, "gt")
        self._on_device(img=img, gt=gt, alpha=alpha, gt_mask=gt_mask, background=background, img_u8=img_u8, gt_u8=gt_u8)
        x, y = f32c(img, "img"), f32c(gt, "gt")
        if x.dim() != 3 or x.shape != y.shape:
            raise ValueError(f"expected two [C,H,W] images of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        C, H, W = x.shape
        a, m = _plane(alpha, "alpha", H, W), _plane(gt_mask, "gt_mask", H, W)
        bg = None
        if background is not None:
            bg = f32c(background, "background")
            if bg.numel() != C:
                raise ValueError(f"background: expected {C} values, got {tuple(bg.shape)}")
        for name, u in (("img_u8", img_u8), ("gt_u8", gt_u8)):
            if u is not None and (u.dtype != torch.uint8 or tuple(u.shape) != (C, H, W) or not u.is_contiguous() or not u.is_cuda):
                raise ValueError(f"{name}: expected a contiguous uint8 [C,H,W] tensor on the device")
        flags = (GSR_PRESENT_CLAMP if clamp else 0) | (GSR_PRESENT_QUANT8 if quantize8 else 0)
        floats = int(lib.gsr_image_metrics_scratch_floats(C, H, W))
        scratch = self._scratch_for(floats)
        with torch.cuda.device(self.device):
            check(lib.gsr_image_metrics(ptr(x), ptr(y), C, H, W, flags, ptr(a), ptr(m), ptr(bg), self._row(v), ptr(scratch), scratch.numel(),
                                        ptr(img_u8), ptr(gt_u8), stream_ptr(self.device)), "gsr_image_metrics")

    def normals(self, v, pred, gt, pred_divisor=1.0, gt_divisor=1.0, eps=1e-8, error_map=None):
        """Row v <- utils/mae_utils.py:3-29 on pred, gt [3,H,W] float32, each divided by its divisor first.  error_map: float32 [H,W]
        that receives the angle in degrees, NaN at invalid pixels."""
        require_cuda(pred, "pred")
        require_cuda(gt, "gt")
        self._on_device(pred=pred, gt=gt, error_map=error_map)
        p, g = f32c(pred, "pred"), f32c(gt, "gt")
        if p.dim() != 3 or p.shape[0] != 3 or p.shape != g.shape:
            raise ValueError(f"expected two [3,H,W] tensors of one shape, got {tuple(p.shape)} and {tuple(g.shape)}")
        H, W = p.shape[1], p.shape[2]
        if error_map is not None and (error_map.dtype != torch.float32 or tuple(error_map.shape) != (H, W) or not error_map.is_contiguous()):
            raise ValueError("error_map: expected a contiguous float32 [H,W] tensor")
        scratch = self._scratch_for(int(lib.gsr_normal_mae_scratch_floats(H, W)))
        with torch.cuda.device(self.device):
            check(lib.gsr_normal_mae(ptr(p), ptr(g), H, W, float(pred_divisor), float(gt_divisor), float(eps), self._row(v), ptr(scratch),
                                     scratch.numel(), ptr(error_map), stream_ptr(self.device)), "gsr_normal_mae")

    def result(self):
        """The table as a float64 numpy array [V, 4]: the one device-to-host copy (it waits for the rows' kernels)."""
        return self.rows.cpu().numpy()


def psnr_from_sums(sse, n):
    """utils/image_utils.py:20-23, 20 log10(1 / sqrt(mse)), from a row's sum of squares and element count; inf for identical images."""
    sse, n = np.asarray(sse, np.float64), np.asarray(n, np.float64)
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(1.0 / np.sqrt(sse / n))


def mae_from_sums(angle_sum, valid, invalid):
    """compute_mae's `angular_error.mean()`: the mean over ALL pixels of a map that holds NaN at the invalid ones, so NaN as soon as
    one pixel is invalid (utils/mae_utils.py:62-64)."""
    angle_sum, valid, invalid = (np.asarray(t, np.float64) for t in (angle_sum, valid, invalid))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(invalid > 0, np.nan, angle_sum / valid)


def evaluate_views(views, pc, pipe, background, gt_normals=None, quantize8=True, keep_images=False):
    """render.py:47-62 followed by metrics.py:67-86 for every view, on the device: render_fast under no_grad, the render clamped to
    [0, 1], both images composited onto `background` where the view has a `gt_alpha_mask`, both quantised to 8 bits (quantize8: what
    the PNG round trip of the reference's two scripts does), then PSNR and SSIM of the presented pair.  One fused kernel per view after
    the render, one read-back after the last view.

    Returns {"PSNR", "SSIM": means over the views, "per_view": {"PSNR": [...], "SSIM": [...]}} and, with gt_normals (one [3,H,W] tensor
    per view, compared with the view's "rend_normal" as utils/mae_utils.angular_error_map does), "MAE" (mean over the views of the
    per-view mean angular error in degrees; a view with an invalid pixel is NaN, as in the reference) and "per_view"["MAE"]; with
    keep_images (quantize8 only) "images": a list of (render, ground truth) uint8 [C,H,W] tensors, what render.py saves as PNGs.
    LPIPS is not provided (see the module docstring)."""
    from gaussian_renderer import render_fast
    views = list(views)
    if keep_images and not quantize8:
        raise ValueError("keep_images returns the 8-bit images and needs quantize8=True")
    if gt_normals is not None and len(gt_normals) != len(views):
        raise ValueError("gt_normals: one tensor per view")
    dev = pc.get_xyz.device
    table = MetricsTable(len(views), dev)
    ntable = MetricsTable(len(views), dev) if gt_normals is not None else None
    images = []
    with torch.no_grad():
        for i, view in enumerate(views):
            pkg = render_fast(view, pc, pipe, background)
            gt = view.original_image[0:3, :, :]
            mask = getattr(view, "gt_alpha_mask", None)
            u8 = None
            if keep_images:
                u8 = (torch.empty(gt.shape, dtype=torch.uint8, device=dev), torch.empty(gt.shape, dtype=torch.uint8, device=dev))
                images.append(u8)
            table.image(i, pkg["render"], gt, clamp=True, alpha=pkg["rend_alpha"] if mask is not None else None, gt_mask=mask,
                        background=background if mask is not None else None, quantize8=quantize8,
                        img_u8=u8[0] if u8 else None, gt_u8=u8[1] if u8 else None)
            if ntable is not None:
                ntable.normals(i, pkg["rend_normal"], gt_normals[i])
    rows = table.result()
    psnrs = psnr_from_sums(rows[:, 0], rows[:, 3])
    ssims = rows[:, 2] / rows[:, 3]
    out = {"PSNR": float(np.mean(psnrs)) if len(views) else math.nan, "SSIM": float(np.mean(ssims)) if len(views) else math.nan,
           "per_view": {"PSNR": [float(p) for p in psnrs], "SSIM": [float(s) for s in ssims]}}
    if ntable is not None:
        nrows = ntable.result()
        maes = mae_from_sums(nrows[:, 0], nrows[:, 1], nrows[:, 2])
        out["MAE"] = float(np.mean(maes)) if len(views) else math.nan
        out["per_view"]["MAE"] = [float(m) for m in maes]
    if keep_images:
        out["images"] = images
    return out
