"""Timing aid (not a test; needs a GPU): one 1080 x 1920 viewer frame as bytes, [H, W, 3] uint8 on the device, two ways, for the modes
RGB, normal, depth and curvature:

  fused   utils.image_utils.present_bytes: one gsr_present_view call (csrc/gsr_viewer.hip), two kernels for a colour-mapped mode
  torch   the reference's chain on the same GPU (tests/viewer_ref.py restates it): the affine, gradient_map's six conv2d calls,
          colormap's two global reductions, normalise, round, gather and permute, then clamp, times 255, .byte(), permute, contiguous

The project had no such function before, so the torch chain is the yardstick.  Calls alternate in one process on one device after a
warm-up, each timed with device events; prints one JSON line with the median and minimum of each.

    timeout -k 10 240 python tests/viewer_present_timing.py [--repeats N] [--warmup W]
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
import viewer_ref as VR  # noqa: E402

MODES = ("RGB", "Normal", "Depth", "Curvature")


def torch_chain_gpu(rgb_out, pkg, items, mode, table):
    """viewer_ref.torch_chain on device tensors, without its guards: what the reference's viewer loop runs per frame."""
    import torch.nn.functional as F
    key, _, half, sobel, repeated = VR.MODES.get(items[mode].lower(), (None, 3, False, False, False))
    img = rgb_out if key is None else pkg[key]
    if half:
        img = (img + 1) / 2
    if sobel:
        kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]).reshape(1, 1, 3, 3).cuda() / 4
        ky = torch.tensor([[-1.0, -2.0, -1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 1.0]]).reshape(1, 1, 3, 3).cuda() / 4
        gx = torch.cat([F.conv2d(img[c][None], kx, padding=1) for c in range(img.shape[0])])
        gy = torch.cat([F.conv2d(img[c][None], ky, padding=1) for c in range(img.shape[0])])
        img = torch.sqrt(gx ** 2 + gy ** 2).norm(dim=0, keepdim=True)
    if repeated:
        img = img.repeat(3, 1, 1)
    if img.shape[0] == 1:
        m = (img - img.min()) / (img.max() - img.min())
        img = table[(m * 255).round().long().squeeze()].permute(2, 0, 1)
    return (torch.clamp(img, min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from utils.image_utils import present_bytes
    H, W = VR.FULL_SIZE
    rgb, pkg = VR.package("normals", H, W, 11)
    pkg["surf_depth"] = VR.image("smooth", 1, H, W, 5)
    rgb = VR.image("smooth", 3, H, W, 6)
    drgb = torch.from_numpy(rgb).cuda()
    dpkg = {k: torch.from_numpy(v).cuda() for k, v in pkg.items()}
    table = torch.from_numpy(VR.turbo()).cuda()
    out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    fns = {}
    for name in MODES:
        mode = VR.ITEMS.index(name)
        fns[name + "_fused"] = lambda mode=mode: present_bytes(drgb, dpkg, VR.ITEMS, mode, out=out)
        fns[name + "_torch"] = lambda mode=mode: torch_chain_gpu(drgb, dpkg, VR.ITEMS, mode, table)
    for _ in range(args.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = {"what": "1080x1920 viewer frame as uint8 [H,W,3]: device-event ms per frame, alternating calls (median and min of repeats)",
           "repeats": args.repeats}
    for name in MODES:
        a, b = fns[name + "_fused"]().clone(), fns[name + "_torch"]()
        res[name + "_differing_bytes"] = int((a != b).sum())
        for k in (name + "_fused", name + "_torch"):
            res[k + "_ms_p50"] = round(float(np.median(ms[k])), 4)
            res[k + "_ms_min"] = round(float(np.min(ms[k])), 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
