"""Image metrics of the reference's utils/image_utils.py on the HIP path: `mse`, `psnr` and `psnr_map`, with the reference's names,
call shapes ([B,C,H,W] -> [B,1]) and formula, so that `from utils.image_utils import psnr` (train.py, metrics.py) resolves here.

Under torch.no_grad(), or when neither image needs a gradient, mse / psnr of two float32 device tensors of one shape run the fused
metrics kernel (csrc/gsr_metrics.hip through gsr_eval.MetricsTable, no presentation step): one launch per image and no elementwise
temporaries.  Dim 0 is the batch whatever the rank, as in the reference: train.py's `psnr(image, gt)` on [3, H, W] gives [3, 1].
When a gradient is required they are the plain torch expression of the reference, which autograd differentiates, and so they are
for what the kernel cannot read as it is: tensors in host memory, other dtypes, shapes that only broadcast; psnr_map is plain torch
always.

Out of scope: `colormap`, `render_net_image`, `plot_cubemap`, `gradient_map` and `to_3ch` of the reference module belong to its
interactive viewer (matplotlib, torchvision) and are not provided.
"""
import torch

from gsr_eval import MetricsTable


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
