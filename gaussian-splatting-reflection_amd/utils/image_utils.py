"""The reference's utils/image_utils.py on the HIP path, with its names and call shapes, so that
`from utils.image_utils import plot_cubemap, psnr, render_net_image` (train.py, view.py, metrics.py) resolves here.

Metrics: `mse`, `psnr` ([B,C,H,W] -> [B,1]) and `psnr_map`.  Under torch.no_grad(), or when neither image needs a gradient, mse /
psnr of two float32 device tensors of one shape run the fused metrics kernel (csrc/gsr_metrics.hip through gsr_eval.MetricsTable,
no presentation step): one launch per image and no elementwise temporaries.  Dim 0 is the batch whatever the rank, as in the
reference: train.py's `psnr(image, gt)` on [3, H, W] gives [3, 1].  When a gradient is required they are the plain torch expression
of the reference, which autograd differentiates, and so they are for what the kernel cannot read as it is: tensors in host memory,
other dtypes, shapes that only broadcast; psnr_map is plain torch always.

Viewer presentation: `render_net_image`, `colormap`, `gradient_map` and the new `present_bytes` run csrc/gsr_viewer.hip
(gsr_present_view): the affine of the normal modes, the Sobel magnitude, the colour map and the 8-bit frame in one kernel, two for
a colour-mapped mode.  The turbo table is utils/turbo_lut.txt (matplotlib's data: 256 rows of three doubles, read as float32 [256, 3]); neither matplotlib nor
torchvision is imported.  These are inference helpers: inputs are detached, the calls run on the current stream and never
synchronise, and there is no torch fallback.  `plot_cubemap` (the 4 x 3 cross, without torchvision) and `to_3ch` are plain torch
copies as in the reference.

Defined where the reference is not:
  * a map whose max equals its min is colour-mapped to index 0 everywhere (the reference divides by zero and indexes with garbage);
  * a NaN gives byte 0 in the 8-bit frame (as torch does on the CPU); under a colour map it takes no part in min and max and gets
    index 0 (the reference raises an index error).
"""
import os

import numpy as np
import torch

from _gsr import GSR_VIEW_COLORMAP, GSR_VIEW_HALF, GSR_VIEW_SOBEL, check, f32c, lib, ptr, require_cuda, require_entry, stream_ptr
from gsr_eval import MetricsTable

require_entry(lib, "gsr_present_view")       # the viewer presentation

TURBO_LUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "turbo_lut.txt")


def _as_images(t):
    """A tensor of any rank as [B, C, H, W] with dim 0 the batch, as the reference's `view(img1.shape[0], -1)` reads it: the last two
    dims are the image, what lies between them and dim 0 the channels.  train.py calls psnr on [3, H, W] (three one-channel images,
    a [3, 1] result)."""
    B = t.shape[0]
    if t.dim() >= 3:
        return t.reshape(B, -1, t.shape[-2], t.shape[-1])
    return t.reshape(B, 1, 1, -1)


def _sum_sq(img1, img2):
    """[B, 1] float64 sums of squared differences and the element count per image, on the device (no host synchronisation)."""
    x, y = _as_images(img1), _as_images(img2)
    B = x.shape[0]
    table = MetricsTable(B, x.device)
    for b in range(B):
        table.image(b, x[b], y[b])
    return table.rows[:, 0:1], table.rows[:, 3:4]


def _on_kernel(img1, img2):
    """The kernel takes what it can read as it is: two float32 device tensors of one shape and one device, no gradient required.
    Everything else the reference's expression accepts (host tensors, other dtypes, shapes that broadcast, empty tensors, a required
    gradient) is evaluated by that expression."""
    if not (img1.is_cuda and img2.is_cuda and img1.device == img2.device and img1.shape == img2.shape):
        return False
    if img1.dtype != torch.float32 or img2.dtype != torch.float32 or img1.dim() < 1 or img1.numel() == 0:
        return False
    if img1.dim() >= 3 and img1.numel() // (img1.shape[0] * img1.shape[-1] * img1.shape[-2]) > 65535:
        return False          # (the channels are a grid dimension of the kernel)
    return not (torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad))


def mse(img1, img2):
    # utils/image_utils.py:17-18
    if not _on_kernel(img1, img2):
        return (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    sse, n = _sum_sq(img1, img2)
    return (sse / n).to(torch.float32)


def psnr(img1, img2):
    # utils/image_utils.py:20-23: [B, C, H, W] -> [B, 1]; identical images give inf
    if not _on_kernel(img1, img2):
        m = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
        return 20 * torch.log10(1.0 / torch.sqrt(m))
    sse, n = _sum_sq(img1, img2)
    return (20 * torch.log10(1.0 / torch.sqrt(sse / n))).to(torch.float32)


def psnr_map(img1, img2):
    # utils/image_utils.py:25-29: [B, C, H, W] -> [B, 1, H, W], the mean over the channels per pixel
    m = torch.mean(((img1 - img2)) ** 2, dim=1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(m))


# ------------------------------------------------------------------------------------------------------- viewer presentation
_tables = {}       # device -> the turbo table there
_scratch = {}      # (device, stream) -> float32 scratch of gsr_present_view: calls on one stream run in order


def _table(cmap, device):
    """The float32 [256, 3] colour table on `device`: "turbo" (utils/turbo_lut.txt) or a caller's tensor."""
    if isinstance(cmap, torch.Tensor):
        require_cuda(cmap, "cmap")
        if cmap.dtype != torch.float32 or tuple(cmap.shape) != (256, 3) or cmap.device != device:
            raise ValueError(f"cmap: expected a float32 [256, 3] tensor on {device}, got {cmap.dtype} {tuple(cmap.shape)} on {cmap.device}")
        return cmap.detach().contiguous()
    if device not in _tables:
        _tables[device] = torch.from_numpy(np.loadtxt(TURBO_LUT, dtype=np.float64).astype(np.float32)).to(device)
    return _tables[device]


def _image(t, name):
    """A detached contiguous float32 [C, H, W] device tensor with C in {1, 3}, or an error before any device call."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.dim() != 3 or t.shape[0] not in (1, 3) or t.numel() == 0:
        raise ValueError(f"{name}: expected a non-empty [C, H, W] tensor with C = 1 or 3, got {tuple(t.shape)}")
    t = f32c(t.detach(), name)
    require_cuda(t, name)
    return t


def _present(src, flags, cmap="turbo", want_f32=True, out_u8=None, want_u8=False):
    """One gsr_present_view call on an _image(); returns (float image or None, uint8 [H, W, 3] or None)."""
    C, H, W = src.shape
    dev = src.device
    table = _table(cmap, dev) if flags & GSR_VIEW_COLORMAP else None
    if out_u8 is not None:
        if (not isinstance(out_u8, torch.Tensor) or out_u8.dtype != torch.uint8 or tuple(out_u8.shape) != (H, W, 3) or not out_u8.is_contiguous()
                or out_u8.device != dev):
            raise ValueError(f"out: expected a contiguous uint8 [{H}, {W}, 3] tensor on {dev}")
    elif want_u8:
        out_u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    out_f32 = None
    if want_f32:
        cout = 3 if (flags & GSR_VIEW_COLORMAP or (C == 3 and not flags & GSR_VIEW_SOBEL)) else 1
        out_f32 = torch.empty((cout, H, W), dtype=torch.float32, device=dev)
    floats = int(lib.gsr_present_view_scratch_floats(C, H, W, flags))
    scratch = None
    if floats:
        key = (dev, stream_ptr(dev))
        scratch = _scratch.get(key)
        if scratch is None or scratch.numel() < floats:
            scratch = _scratch[key] = torch.empty(floats, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.gsr_present_view(ptr(src), C, H, W, flags, ptr(table), ptr(out_f32), ptr(out_u8), ptr(scratch),
                                   0 if scratch is None else scratch.numel(), stream_ptr(dev)), "gsr_present_view")
    return out_f32, out_u8


def gradient_map(image):
    # utils/image_utils.py:33-42: [C, H, W] -> [1, H, W], the Sobel magnitude (zero padding) normed over the channels
    return _present(_image(image, "image"), GSR_VIEW_SOBEL)[0]


def colormap(map, cmap="turbo"):
    # utils/image_utils.py:44-49: [1, H, W] or [H, W] -> [3, H, W]; cmap may also be a float32 [256, 3] device tensor
    if not isinstance(cmap, torch.Tensor) and cmap != "turbo":
        raise NotImplementedError(f"colormap: only 'turbo' (or a [256, 3] tensor) is provided, got {cmap!r}")
    if isinstance(map, torch.Tensor) and map.dim() == 2:
        map = map[None]
    if isinstance(map, torch.Tensor) and map.dim() == 3 and map.shape[0] != 1:
        raise ValueError(f"map: expected [1, H, W] or [H, W], got {tuple(map.shape)}")
    return _present(_image(map, "map"), GSR_VIEW_COLORMAP, cmap)[0]


# mode (lower case) -> (key of the render package, flags, repeated to three channels); anything else shows rgb_out
_MODES = {
    "alpha": ("rend_alpha", 0, False),
    "mask": ("env_scope_mask", 0, True),
    "normal": ("rend_normal", GSR_VIEW_HALF, False),
    "depth": ("surf_depth", 0, False),
    "base color": ("base_color_map", 0, False),
    "refl. strength": ("refl_strength_map", 0, True),
    "refl. color": ("refl_color_map", 0, False),
    "edge": ("surf_normal", GSR_VIEW_HALF, False),
    "curvature": ("rend_normal", GSR_VIEW_HALF | GSR_VIEW_SOBEL, False),
    "rgb raw": ("render", 0, False),
}


def _select(rgb_out, render_pkg, render_items, render_mode):
    """(source image, flags of gsr_present_view, repeated) of a mode, by the reference's rules (utils/image_utils.py:51-84): a mode
    past the end of the list is mode 0; a package without the mode's key raises KeyError; only a one-channel result is colour-mapped,
    so the repeated maps ('mask', 'refl. strength') are not."""
    if render_mode >= len(render_items):
        render_mode = 0
    mode = _MODES.get(render_items[render_mode].lower())
    if mode is None:
        return _image(rgb_out, "rgb_out"), 0, False
    key, flags, repeated = mode
    src = _image(render_pkg[key], key)
    if repeated and src.shape[0] != 1:
        raise ValueError(f"{key}: expected [1, H, W], got {tuple(src.shape)}")
    if not repeated and (src.shape[0] == 1 or flags & GSR_VIEW_SOBEL):
        flags |= GSR_VIEW_COLORMAP
    return src, flags, repeated


def render_net_image(rgb_out, render_pkg, render_items, render_mode, camera=None):
    # utils/image_utils.py:51-84: the float image of a viewer mode, [3, H, W].  `camera` is unused, as in the reference.
    src, flags, repeated = _select(rgb_out, render_pkg, render_items, render_mode)
    if repeated:
        return src.repeat(3, 1, 1)
    if flags == 0:
        return src
    return _present(src, flags)[0]


def present_bytes(rgb_out, render_pkg, render_items, render_mode, out=None):
    """The frame the reference's viewer sends (train.py:333-334), uint8 [H, W, 3] on the device:
    (clamp(render_net_image(...), 0, 1) * 255).byte().permute(1, 2, 0).contiguous(), as ONE gsr_present_view call with no float
    intermediate.  `out`: an optional contiguous uint8 [H, W, 3] device tensor to fill (and return)."""
    src, flags, _ = _select(rgb_out, render_pkg, render_items, render_mode)
    return _present(src, flags, want_f32=False, out_u8=out, want_u8=True)[1]


def plot_cubemap(textures):
    """utils/image_utils.py:86-100 without torchvision: six faces [6, C, h, w] as a 4 x 3 cross in a zero [C, 3h, 4w] tensor.  Cell k
    of the grid (row k // 4, column k % 4, what make_grid(nrow=4, padding=0) does) holds: 1 <- face 3 flipped along its first image
    axis, 4 <- face 1, 5 <- face 4, 6 <- face 0, 7 <- face 5, 9 <- face 2.  One-channel faces come out as three channels, as make_grid
    gives them."""
    if len(textures) != 6 or textures[0].dim() != 3:
        raise ValueError("textures: expected six [C, h, w] faces")
    C, h, w = textures[0].shape
    grid = torch.zeros((C, 3 * h, 4 * w), dtype=textures[0].dtype, device=textures[0].device)
    for cell, face in ((1, torch.flip(textures[3], [1])), (4, textures[1]), (5, textures[4]), (6, textures[0]), (7, textures[5]), (9, textures[2])):
        r, c = cell // 4, cell % 4
        grid[:, r * h:(r + 1) * h, c * w:(c + 1) * w] = face
    return grid.repeat(3, 1, 1) if C == 1 else grid


def to_3ch(t):
    """utils/image_utils.py:102-157: an image-like tensor as [B, 3, H, W] in host memory.  Accepts (H, W), (C, H, W), (H, W, C),
    (B, C, H, W) and (B, H, W, C) with C in {1, 3}; one channel is repeated, another channel count is averaged to one and repeated.
    None gives None.  (A 3-D tensor with neither its first nor its last dim in {1, 3} is refused with ValueError; the reference fails
    on it inside torch.)"""
    if t is None:
        return None
    t = t.detach().cpu()
    if t.dim() == 2:
        t = t[None, None]
    elif t.dim() == 3:
        if t.shape[0] in (1, 3):
            t = t[None]
        elif t.shape[2] in (1, 3):
            t = t.permute(2, 0, 1)[None]
        else:
            raise ValueError(f"cannot tell the channel dim of {tuple(t.shape)}")
    elif t.dim() == 4:
        if t.shape[1] not in (1, 3) and t.shape[3] in (1, 3):
            t = t.permute(0, 3, 1, 2)
    else:
        raise ValueError(f"Unsupported tensor dim {t.dim()} for image-like data")
    if t.shape[1] != 3:
        if t.shape[1] != 1:
            t = t.mean(dim=1, keepdim=True)
        t = t.repeat(1, 3, 1, 1)
    return t
