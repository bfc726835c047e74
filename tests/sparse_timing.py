"""Timing aid (not a test; needs a GPU): gsr_mesh.SparseTSDFVolume beside gsr_mesh.TSDFVolume at the layout and size of
tests/mesh_timing.py, and at one size the dense volume cannot hold.

  512^3 equivalent   six 1920 x 1080 views of an analytic ball of radius 2 from 4 units away into the box around the cameras' sphere, as
                     GaussianExtractor.extract_mesh_bounded lays it out.  Per view: sparse touch (walks every block of the box), sparse
                     integrate (the allocated blocks), dense integrate, timed in the same run; then both extractions after six views.
  2048^3 equivalent  the same box at a quarter of the voxel, 8.6e9 nodes: the slots, the bytes of table and pool, and the milliseconds of
                     touch, allocate, integrate and extract.

Each figure is sampled `--repeats` times with device events after a warm-up and reported as median [min, max] in ms (allocate once: it
changes the volume).  A report, not an assertion.

    timeout -k 10 500 python tests/sparse_timing.py [--repeats N] [--warmup W] [--size 512] [--large 2048]
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
import cameras  # noqa: E402
import gsr_synth as S  # noqa: E402
import mesh_ref as M  # noqa: E402
from mesh_timing import DEPTH_TRUNC, RADIUS, SDF_TRUNC, H, W, sample  # noqa: E402


def views():
    """[(depth, camera, rgb)] on the device: mesh_timing.py's six views."""
    staged, rs = [], np.random.RandomState(3)
    for cam in S.circle_cameras(W, H, n=6, radius=4.0):
        depth = M.ray_depth_map(cam, (0.0, 0.0, 0.0), RADIUS, np.array([0.0, 0.0, 1.0]), 1e9)
        depth[depth > 100] = 0
        staged.append((torch.from_numpy(depth).cuda(), cameras.view_of(cam), torch.from_numpy(rs.rand(3, H, W).astype(np.float32)).cuda()))
    return staged


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, round(e0.elapsed_time(e1), 4)


def sparse_run(n, staged, sdf_trunc, repeats, warmup):
    """Touch, allocate, integrate and extract over the box of n^3 nodes; the figures as a dictionary, and the volume."""
    import gsr_mesh
    voxel, origin = 8.0 / (n - 1), (-4.0, -4.0, -4.0)
    kw = dict(sdf_trunc=sdf_trunc, depth_trunc=DEPTH_TRUNC)
    vol = gsr_mesh.SparseTSDFVolume(origin, voxel, (n, n, n), "cuda", color=True)
    depth, view, rgb = staged[0]
    res = {"nodes": n ** 3, "blocks_in_box": int(vol.table.numel())}
    res["touch"] = sample(lambda: vol.touch(depth, view, **kw), repeats, warmup)
    for depth_k, view_k, _ in staged:
        vol.touch(depth_k, view_k, **kw)
    slots, res["allocate_ms"] = once(vol.allocate)
    res["slots"], res["bytes"], res["pool_share_of_box"] = slots, vol.nbytes, round(slots / vol.table.numel(), 5)
    res["integrate"] = sample(lambda: vol.integrate(depth, view, rgb=rgb, **kw), repeats, warmup)
    vol.tsdf.zero_(), vol.weight.zero_(), vol.color.zero_()
    for depth_k, view_k, rgb_k in staged:
        vol.integrate(depth_k, view_k, rgb=rgb_k, **kw)
    mesh = vol.extract()
    res["vertices"], res["faces"] = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    res["median_radius_error"] = round(float((mesh.vertices.norm(dim=1) - RADIUS).abs().median()), 6)
    res["extract"] = sample(vol.extract, repeats, warmup)
    return res, vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--large", type=int, default=2048)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import gsr_mesh
    staged = views()
    n = args.size
    res = {"what": f"{W} x {H} views into {n}^3 with colour, sparse beside dense, and sparse alone at {args.large}^3: device-event ms, median [min, max]",
           "repeats": args.repeats}
    res["sparse"], vol = sparse_run(n, staged, SDF_TRUNC, args.repeats, args.warmup)
    dense = gsr_mesh.TSDFVolume((-4.0, -4.0, -4.0), 8.0 / (n - 1), (n, n, n), "cuda", color=True)
    depth, view, rgb = staged[0]
    res["dense"] = {"bytes": 5 * 4 * n ** 3}
    res["dense"]["integrate"] = sample(lambda: dense.integrate(depth, view, rgb=rgb, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC), args.repeats, args.warmup)
    dense.reset()
    for depth_k, view_k, rgb_k in staged:
        dense.integrate(depth_k, view_k, rgb=rgb_k, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC)
    mesh = dense.extract()
    res["dense"]["vertices"], res["dense"]["faces"] = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    res["dense"]["extract"] = sample(dense.extract, args.repeats, args.warmup)
    tsdf, weight, _ = vol.to_dense()
    has = weight > 0                                                 # (the sparse planes were fused once per view, as the dense ones)
    res["fused_nodes_equal_dense"] = bool(torch.equal(tsdf[has], dense.tsdf[has]) and torch.equal(weight[has], dense.weight[has]))
    del dense, vol, mesh, has, tsdf, weight
    torch.cuda.empty_cache()
    if args.large:
        # the truncation shrinks with the voxel, as a user of the smaller voxel would set it
        res["large"], _ = sparse_run(args.large, staged, SDF_TRUNC * (n - 1) / (args.large - 1), max(3, args.repeats // 3), 1)
        res["large"]["dense_would_need_bytes"] = 5 * 4 * args.large ** 3
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
