"""MI355X drop-in for the `fused_ssim` package the reference imports (`from fused_ssim import fused_ssim`, train.py:38; its
submodules/fused-ssim directory is empty): the mean of the 11 x 11 Gaussian-window SSIM map of two [B,C,H,W] images, with the
gradient w.r.t. img1, on the kernels of libgsr_hip.so (utils.loss_utils.FusedSSIMMap)."""
from utils.loss_utils import C1, C2, FusedSSIMMap

allowed_padding = ["same", "valid"]


def fused_ssim(img1, img2, padding="same", train=True):
    """"same": the mean of the zero-padded map; "valid": the mean of the map pixels whose window lies inside the image,
    map[:, :, 5:-5, 5:-5].  train=False computes the value alone: nothing is kept for a backward."""
    assert padding in allowed_padding
    smap = FusedSSIMMap.apply(C1, C2, img1 if train else img1.detach(), img2)
    if padding == "valid":
        smap = smap[..., 5:-5, 5:-5]
    return smap.mean()
