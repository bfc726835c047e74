"""Timing aid (not a test; needs a GPU): the unbounded mesh extraction at full size, against the same steps written as whole-lattice torch
ops on the same GPU, which stand in for what upstream's Python does there:

  integrate   one 1920 x 1080 view (an analytic ball of radius 2 on an endless floor, seen from 4 units away) into a lattice of size^3
              nodes in contracted space about the cameras' sphere, as GaussianExtractor.extract_mesh_unbounded lays it out
              fused: ContractedTSDFVolume.integrate, one kernel (csrc/gsr_unbounded.hip);  torch: un-contraction, projection, grid_sample
              of the depth map and of its validity, masked update, each over the whole lattice
  extract     ContractedTSDFVolume.extract after the six views, fused twice each: count, scan, emit, un-contraction, the 16-byte read-back
  colour      color_vertices over the six views on the extracted vertices
  pipeline    all of it once: six integrations, the extraction, the colouring

Each is sampled `--repeats` times with device events after a warm-up and reported as median [min, max] in ms.  Beside the integrate: the
share of the lattice inside the shell (m < 2), the share the view writes, and the time the plane traffic of the written nodes alone
would take (two planes read and written, 16 bytes per written node, at 6.3 TB/s): a node the view does not write costs no plane traffic,
so this figure against the measured time is what a fusion of several views per pass would have to beat — a report, not an assertion.

    timeout -k 10 600 python tests/unbounded_timing.py [--repeats N] [--warmup W] [--sizes 512,1024] [--no-torch]
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
from mesh_timing import sample  # noqa: E402

W, H, BALL, FLOOR, CAMERA_RADIUS, EXTENT = 1920, 1080, 2.0, -6.0, 4.0, 1.9


def torch_integrate(vol, depth, view, proj):
    """include/gsr_hip_unbounded.h, steps 1-5, on whole planes."""
    n, dev = vol.resolution, vol.tsdf.device
    a = vol.lo + vol.step * torch.arange(n, device=dev, dtype=torch.float32)
    yx, yy, yz = a[None, None, :], a[None, :, None], a[:, None, None]
    m = torch.sqrt(yx * yx + yy * yy + yz * yz)
    ok = m < 2
    shell = m > 1
    s = torch.where(shell, 1 / (m * (2 - m)), torch.ones_like(m)) * vol.radius
    trunc = torch.where(shell, 5 * vol.voxel_size / (2 - m.clamp(max=1.9)), torch.full_like(m, 5 * vol.voxel_size))
    X, Y, Z = s * yx + vol.center[0], s * yy + vol.center[1], s * yz + vol.center[2]
    z = view[0, 2] * X + view[1, 2] * Y + view[2, 2] * Z + view[3, 2]
    p = [proj[0, r] * X + proj[1, r] * Y + proj[2, r] * Z + proj[3, r] for r in (0, 1, 3)]
    del X, Y, Z, s
    ok &= (z > 0) & (p[2] > 0)
    qx, qy = p[0] / p[2], p[1] / p[2]
    del p
    ok &= (qx > -1) & (qx < 1) & (qy > -1) & (qy < 1)
    grid = torch.stack([qx, qy], -1).reshape(1, n, n * n, 2)          # align_corners=False: pixel u is centred on ((2 u + 1) / W - 1)
    del qx, qy
    maps = torch.stack([depth, (depth > 0).float()])[None]
    got = torch.nn.functional.grid_sample(maps, grid, mode="bilinear", padding_mode="border", align_corners=False).reshape(2, n, n, n)
    del grid
    ok &= got[1] >= 1                                                  # every tap carries a depth
    sdf = got[0] - z
    ok &= sdf > -trunc
    t = (sdf / trunc).clamp(-1, 1)
    w1 = vol.weight + 1
    vol.tsdf.copy_(torch.where(ok, (vol.tsdf * vol.weight + t) / w1, vol.tsdf))
    vol.weight.copy_(torch.where(ok, w1, vol.weight))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import gsr_mesh
    cams = S.circle_cameras(W, H, n=6, radius=CAMERA_RADIUS)
    staged = []
    rs = np.random.RandomState(3)
    for cam in cams:
        depth = M.ray_depth_map(cam, (0.0, 0.0, 0.0), BALL, np.array([0.0, 1.0, 0.0]), FLOOR)
        depth[depth > 100] = 0
        staged.append((cameras.view_of(cam), torch.from_numpy(depth).cuda(), torch.from_numpy(rs.rand(3, H, W).astype(np.float32)).cuda()))
    centres = np.stack([c["campos"] for c in cams]).astype(np.float64)
    centre = centres.mean(0)
    radius = float(np.linalg.norm(centres - centre, axis=1).max())
    for n in (int(s) for s in args.sizes.split(",")):
        vol = gsr_mesh.ContractedTSDFVolume(centre, radius, n, EXTENT, "cuda")
        res = {"what": f"{W} x {H} views into a contracted lattice of {n}^3, extent {EXTENT}: device-event ms, median [min, max]", "size": n,
               "repeats": args.repeats, "depth_share": round(float((staged[0][1] > 0).float().mean()), 4)}
        view, depth, rgb = staged[0]
        fused = lambda: vol.integrate(depth, view)
        res["integrate_fused"] = sample(fused, args.repeats, args.warmup)
        vol.reset()
        fused()
        written = float((vol.weight > 1).float().mean())
        a = vol.lo + vol.step * torch.arange(n, device="cuda", dtype=torch.float32)
        live = float(((a * a)[None, None, :] + (a * a)[None, :, None] + (a * a)[:, None, None] < 4).float().mean())
        res["lattice_share_inside_the_shell"], res["integrate_written_share"] = round(live, 4), round(written, 4)
        res["integrate_plane_bytes_of_written_nodes"] = int(written * n ** 3 * 16)
        res["integrate_byte_floor_ms"] = round(written * n ** 3 * 16 / 6.3e12 * 1e3, 4)
        res["integrate_bytes_if_every_node_were_read_and_written_ms"] = round(n ** 3 * 16 / 6.3e12 * 1e3, 4)
        if not args.no_torch:
            chain = lambda: torch_integrate(vol, depth, view.world_view_transform, view.full_proj_transform)
            before = vol.weight.clone()
            chain()
            res["integrate_torch_weight_mismatches"] = int((vol.weight != before + (before > 1)).sum())      # the chain writes the same nodes
            del before
            res["integrate_torch"] = sample(chain, max(3, args.repeats // 3), 1)
            torch.cuda.empty_cache()

        def fuse_all():
            for _ in range(2):
                for view, depth, _ in staged:
                    vol.integrate(depth, view)
        vol.reset()
        fuse_all()
        mesh = vol.extract()
        res["extract_vertices"], res["extract_faces"] = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
        res["extract_fused"] = sample(vol.extract, args.repeats, args.warmup)
        views = [(view, depth, rgb) for view, depth, rgb in staged]
        res["colour_six_views"] = sample(lambda: gsr_mesh.color_vertices(mesh.vertices, views, 5.0 * vol.voxel_size), args.repeats, args.warmup)

        def pipeline():
            vol.reset()
            fuse_all()
            m = vol.extract()
            return gsr_mesh.color_vertices(m.vertices, views, 5.0 * vol.voxel_size)
        res["pipeline_twelve_integrations_extract_colour"] = sample(pipeline, max(3, args.repeats // 3), 1)
        print(json.dumps(res), flush=True)
        del vol, mesh
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
