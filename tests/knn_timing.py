"""Timing aid (not a test; needs a GPU): simple_knn.distCUDA2 (csrc/gsr_knn.hip) at P = 1e5, 1e6 and 5e6 on three clouds — uniform in a
cube, tight clusters with 1 % far outliers, and the NeRF-synthetic start (uniform in [-1.3, 1.3]^3) — timed with device events after a
warm-up, median of the repeats; and, as the CPU baseline, scipy's cKDTree (build + k = 4 query, 16 workers) on the same points.  Prints
one JSON line.

    python tests/knn_timing.py [--repeats N] [--warmup W] [--sizes 100000,1000000,5000000] [--kinds uniform,clusters,nerf] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_knn import _cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000,5000000")
    ap.add_argument("--kinds", default="uniform,clusters,nerf")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from simple_knn._C import distCUDA2
    out = {"what": "distCUDA2 device-event ms (median of repeats after warm-up) and host cKDTree ms (16 workers)", "repeats": args.repeats}
    names = {"uniform": "uniform", "clusters": "clustered_outliers", "nerf": "nerf_synthetic"}
    for kind in args.kinds.split(","):
        name = names[kind]
        for P in (int(s) for s in args.sizes.split(",")):
            pts = _cloud(kind, P, 1000 + P)
            x = torch.from_numpy(pts).cuda()
            for _ in range(args.warmup):
                distCUDA2(x)
            ms = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                distCUDA2(x)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            rec = {"gpu_ms_p50": round(float(np.median(ms)), 4), "gpu_ms_min": round(float(np.min(ms)), 4)}
            if not args.no_cpu:
                from scipy.spatial import cKDTree
                a = time.perf_counter()
                cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4, workers=16)
                rec["ckdtree_ms"] = round((time.perf_counter() - a) * 1e3, 1)
            out["%s_%d" % (name, P)] = rec
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
