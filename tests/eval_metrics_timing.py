"""Timing aid (not a test; needs a GPU): the three evaluation sums of one 3 x 1080 x 1920 view — sum (v - g)^2, sum |v - g|, sum ssim —
two ways, with the full presentation (clamp, composite with alpha and mask, 8-bit quantisation):

  fused     one gsr_image_metrics call (csrc/gsr_metrics.hip) into a table row
  composed  what the library offered before it: torch elementwise presentation ops (about twenty small launches), gsr_ssim_l1_forward
            called through the C ABI with the backward's three planes as outputs (what the training path runs for an image that
            requires a gradient), and a torch sum of squares.  At this size those launches are short: part of the composed time is
            launch overhead between them, not device work

Calls alternate in one process on one device, each timed with device events after a warm-up; prints one JSON line with the median and
minimum of each.

    python tests/eval_metrics_timing.py [--repeats N] [--warmup W]
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
import metrics_ref as MR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from _gsr import check, lib, ptr, stream_ptr
    from gsr_eval import MetricsTable
    shape = MR.FULL_SIZE
    C, H, W = shape
    v, g = MR.image_pair("uniform", shape, 3)
    kw = MR.presentation_inputs("clamp_composite_quantize", shape, 3)
    V, G, A, M, BG = (torch.from_numpy(t).cuda() for t in (v, g, kw["alpha"], kw["gt_mask"], kw["background"]))
    table = MetricsTable(1, "cuda")
    sums = torch.empty(2, device="cuda")
    planes = torch.empty((3, C, H, W), device="cuda")
    scratch = torch.empty(int(lib.gsr_ssim_l1_scratch_floats(C, H, W)), device="cuda")
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def fused():
        table.image(0, V, G, clamp=True, alpha=A, gt_mask=M, background=BG, quantize8=True)

    def composed():
        x = torch.clamp(V, 0.0, 1.0)
        a = torch.clamp(A, 0.0, 1.0)[None]
        x = x * a + (1 - a) * BG[:, None, None]
        y = G * M[None] + (1 - M[None]) * BG[:, None, None]
        x = x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).to(torch.float32).div_(255)
        y = y.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).to(torch.float32).div_(255)
        check(lib.gsr_ssim_l1_forward(ptr(x), ptr(y), C, H, W, c1, c2, ptr(sums), ptr(scratch), None, ptr(planes[0]), ptr(planes[1]), ptr(planes[2]),
                                      stream_ptr(x.device)), "gsr_ssim_l1_forward")
        return ((x - y) ** 2).sum()

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
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    sse = float(composed())
    row = table.result()[0]
    out = {"what": "3x1080x1920, clamp + composite + quantise: device-event ms per view, alternating calls (median and min of repeats)",
           "repeats": args.repeats, "agree": bool(abs(row[0] - sse) <= 1e-5 * sse and abs(row[2] - float(sums[1])) <= 1e-5 * abs(row[2]))}
    for k in fns:
        out[k + "_ms_p50"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min"] = round(float(np.min(ms[k])), 4)
    out["fused_bytes_per_pixel_channel"] = round((2 * 4 * C + 2 * 4) / C, 2)       # two images + the alpha and mask planes
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
