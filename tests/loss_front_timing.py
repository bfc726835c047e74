"""Timing aid (not a test; needs a GPU): forward + backward of the photometric loss of one 3 x 1080 x 1920 view that carries a
gt_alpha_mask, with gradients to the render and to its alpha plane, two ways:

  fused     photometric_loss(rgb, gt, lambda, alpha=, gt_alpha_mask=, background=): the composites are formed inside
            gsr_photometric_forward / _backward (csrc/gsr_loss.hip)
  composed  what it replaces: the torch compositing of train.py:158-159 (about ten elementwise launches, and their autograd twins
            on the way back), then photometric_loss on the two finished images (gsr_ssim_l1_forward / _backward)

Calls alternate in one process on one device after a warm-up; a sample is `--inner` forward + backward passes between two device
events, and the figures are per pass.  Prints one JSON line with the median and minimum of each, and whether the two agree.

    python tests/loss_front_timing.py [--repeats N] [--inner K] [--warmup W]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import loss_front_bounds as FB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=(3, 1080, 1920), metavar=("C", "H", "W"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_front_timing.py measures on the GPU; none is available")
    from utils.loss_utils import clear_cache, photometric_loss
    shape = tuple(args.size)
    C, H, W = shape
    lam = 0.2
    rs = np.random.RandomState(3)
    gt = rs.rand(*shape).astype(np.float32)
    rgb = (0.6 * gt + 0.4 * rs.rand(*shape)).astype(np.float32)
    RGB, GT = torch.from_numpy(rgb).cuda().requires_grad_(True), torch.from_numpy(gt).cuda()
    A = torch.from_numpy(FB.alpha_plane("noise", H, W, 3)).cuda()[None].requires_grad_(True)
    M = torch.from_numpy(FB.mask_plane("binary", H, W, 3)).cuda()[None]
    BG = torch.tensor(FB.BACKGROUNDS[2], device="cuda")

    def fused():
        RGB.grad = A.grad = None
        loss = photometric_loss(RGB, GT, lam, alpha=A, gt_alpha_mask=M, background=BG)
        loss.backward()
        return loss

    def composed():
        RGB.grad = A.grad = None
        gt_image = GT * M + (1 - M) * BG[:, None, None]
        image = RGB * A + (1 - A) * BG[:, None, None]
        loss = photometric_loss(image, gt_image, lam)
        loss.backward()
        return loss

    fns = {"fused": fused, "composed": composed}
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.inner)
    res = {}
    for k, f in fns.items():
        loss = f()
        res[k] = (loss.item(), RGB.grad.clone(), A.grad.clone())
    clear_cache()
    (lf, gf, af), (lc, gc, ac) = res["fused"], res["composed"]
    agree = (abs(lf - lc) <= 1e-6 and (gf - gc).abs().max().item() <= 1e-5 * gc.abs().max().item()
             and (af - ac).abs().max().item() <= 1e-5 * ac.abs().max().item())
    out = {"what": "%dx%dx%d photometric loss with alpha and mask, forward + backward to rgb and alpha: device-event ms per pass, "
                   "alternating calls (median and min of repeats)" % shape,
           "repeats": args.repeats, "inner": args.inner, "agree": bool(agree)}
    for k in fns:
        out[k + "_ms_p50"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min"] = round(float(np.min(ms[k])), 4)
    # global traffic of the fused kernels per pixel-channel, 4-byte words: forward rgb, gt (+ alpha, mask per pixel) in, three planes
    # out; backward three planes, rgb, gt (+ alpha, mask) in, dL/drgb (+ dL/dalpha) out
    out["fused_bytes_per_pixel_channel"] = round(4 * ((2 * C + 2 + 3 * C) + (5 * C + 2 + C + 1)) / C, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
