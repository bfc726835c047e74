"""Stand-in for the reference's pybind module `simple_knn._C`: distCUDA2(points), implemented over the C ABI of libgsr_hip.so
(gsr_knn_mean_dist, include/gsr_hip.h).

distCUDA2(points) -> (P,) float32 on the points' device: element i is the mean of the squared distances from point i to its 3
nearest other points (a missing neighbour, P < 4, counts as FLT_MAX).  The search is exact and the result does not depend on the
input order.  Runs on the current torch stream without a host synchronisation; output and scratch come from torch.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _gsr  # noqa: E402
from _gsr import check, f32c, lib, ptr, stream_ptr  # noqa: E402

_gsr.require_entry(lib, "gsr_knn_mean_dist")


def distCUDA2(points):
    if not isinstance(points, torch.Tensor):
        raise ValueError("distCUDA2: points must be a tensor on a GPU")
    if points.dim() != 2 or points.size(1) != 3:
        raise ValueError(f"distCUDA2: points must have shape (P, 3), got {tuple(points.shape)}")
    pts = f32c(points, "points")
    if not pts.is_cuda:
        raise ValueError("distCUDA2: points must be a tensor on a GPU")
    P = pts.size(0)
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    nbytes = int(lib.gsr_knn_scratch_bytes(P))
    if nbytes == 0:
        raise ValueError(f"distCUDA2: {P} points, at most 2^30 - 1 are supported")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    with torch.cuda.device(pts.device):
        check(lib.gsr_knn_mean_dist(P, ptr(pts), ptr(out), ptr(scratch), nbytes, stream_ptr(pts.device)), "gsr_knn_mean_dist")
    return out
