"""Timing aid (not a test; needs a GPU): the two halves of gsr_mesh at full size, each against the same arithmetic written as a torch op
chain on the same GPU (the project had neither before, so the chain is the yardstick):

  integrate   one 1920 x 1080 view (an analytic ball of radius 2 seen from 4 units away) into a 512^3 volume with colour over the box
              around the cameras' sphere, as GaussianExtractor.extract_mesh_bounded lays it out: the camera sits on a face of the box
              fused: TSDFVolume.integrate, one kernel (csrc/gsr_mesh.hip);  torch: the header's steps 1-5 as whole-volume tensor ops
  extract     the iso-surface of that volume after six views round the ball
              fused: TSDFVolume.extract (classify, count, scan, offsets, emit, and the 16-byte read-back);  torch: classification, cell
              validity, the seven edge masks, nonzero and the interpolation — the vertex half only, it emits no faces, so the chain does
              LESS than the kernels

Each is sampled `--repeats` times with device events after a warm-up and reported as median [min, max] in ms.  Beside the integrate:
the share of nodes the view observes and the time their plane traffic alone would take (five planes read and written, 40 bytes per
observed node, at 6.3 TB/s) — a report, not an assertion.  GSR_LIB selects another build of the library (tests/ab_build.py) for an A/B
of a -D variant of csrc/gsr_mesh.hip.

    timeout -k 10 400 python tests/mesh_timing.py [--repeats N] [--warmup W] [--size 512] [--no-torch]
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

W, H, RADIUS, SDF_TRUNC, DEPTH_TRUNC = 1920, 1080, 2.0, 0.05, 8.0
DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


def torch_integrate(tsdf, weight, color, origin, voxel, depth, rgb, view, proj):
    """include/gsr_hip_mesh.h, steps 1-5, on whole planes."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    X = (origin[0] + voxel * torch.arange(nx, device=dev, dtype=torch.float32))[None, None, :]
    Y = (origin[1] + voxel * torch.arange(ny, device=dev, dtype=torch.float32))[None, :, None]
    Z = (origin[2] + voxel * torch.arange(nz, device=dev, dtype=torch.float32))[:, None, None]
    z = view[0, 2] * X + view[1, 2] * Y + view[2, 2] * Z + view[3, 2]
    p = [proj[0, r] * X + proj[1, r] * Y + proj[2, r] * Z + proj[3, r] for r in (0, 1, 3)]
    ok = (z > 0) & (p[2] > 0)
    u = torch.round(((p[0] / p[2] + 1) * W - 1) / 2)
    v = torch.round(((p[1] / p[2] + 1) * H - 1) / 2)
    ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
    pix = (v.clamp(0, H - 1) * W + u.clamp(0, W - 1)).long()
    d = depth.reshape(-1)[pix]
    ok &= (d > 0) & (d <= DEPTH_TRUNC)
    sdf = d - z
    ok &= sdf >= -SDF_TRUNC
    t = torch.clamp(sdf / SDF_TRUNC, max=1.0)
    w1 = weight + 1
    tsdf.copy_(torch.where(ok, (tsdf * weight + t) / w1, tsdf))
    for c in range(3):
        color[c].copy_(torch.where(ok, (color[c] * weight + rgb[c].reshape(-1)[pix]) / w1, color[c]))
    weight.copy_(torch.where(ok, w1, weight))


def torch_extract_vertices(tsdf, weight, origin, voxel, min_weight=1.0):
    """tests/mesh_ref.py extract_vertices as torch ops: the vertex half of the extraction."""
    nz, ny, nx = tsdf.shape
    valid, inside = weight >= min_weight, tsdf < 0
    ok = torch.ones((nz - 1, ny - 1, nx - 1), dtype=torch.bool, device=tsdf.device)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ok &= valid[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    cells = torch.zeros((nz + 1, ny + 1, nx + 1), dtype=torch.bool, device=tsdf.device)
    cells[1:-1, 1:-1, 1:-1] = ok
    o = torch.tensor(origin, device=tsdf.device)
    out = []
    for dx, dy, dz in DIRS:
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        held = torch.zeros_like(valid[lo])
        for oz in ((1,) if dz else (0, 1)):
            for oy in ((1,) if dy else (0, 1)):
                for ox in ((1,) if dx else (0, 1)):
                    held |= cells[oz:oz + nz - dz, oy:oy + ny - dy, ox:ox + nx - dx]
        k, j, i = torch.nonzero(valid[lo] & valid[hi] & (inside[lo] != inside[hi]) & held, as_tuple=True)
        ta, tb = tsdf[k, j, i], tsdf[k + dz, j + dy, i + dx]
        f = ta / (ta - tb)
        a = o + voxel * torch.stack([i, j, k], 1).float()
        out.append(a + voxel * torch.tensor([dx, dy, dz], device=tsdf.device).float() * f[:, None])
    return torch.cat(out)


def sample(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_p50": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import gsr_mesh
    n = args.size
    # the layout GaussianExtractor.extract_mesh_bounded gives: the box around the sphere that holds the camera centres
    voxel = 8.0 / (n - 1)
    origin = (-4.0, -4.0, -4.0)
    cams = S.circle_cameras(W, H, n=6, radius=4.0)
    staged = []
    rs = np.random.RandomState(3)
    for cam in cams:
        depth = M.ray_depth_map(cam, (0.0, 0.0, 0.0), RADIUS, np.array([0.0, 0.0, 1.0]), 1e9)
        depth[depth > 100] = 0
        staged.append((torch.from_numpy(depth).cuda(), cameras.view_of(cam), torch.from_numpy(rs.rand(3, H, W).astype(np.float32)).cuda()))
    vol = gsr_mesh.TSDFVolume(origin, voxel, (n, n, n), "cuda", color=True)
    res = {"what": f"{W} x {H} view into {n}^3 with colour, and the extraction after six views: device-event ms, median [min, max]",
           "repeats": args.repeats, "lib": os.environ.get("GSR_LIB", "default")}
    depth, view, rgb = staged[0]
    fused = lambda: vol.integrate(depth, view, rgb=rgb, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC)
    res["integrate_fused"] = sample(fused, args.repeats, args.warmup)
    vol.reset()
    fused()
    observed = float((vol.weight > 0).float().mean())
    res["integrate_observed_share"] = round(observed, 4)
    res["integrate_byte_floor_ms"] = round(observed * n ** 3 * 40 / 6.3e12 * 1e3, 4)
    if not args.no_torch:
        chain = lambda: torch_integrate(vol.tsdf, vol.weight, vol.color, origin, voxel, depth, rgb, view.world_view_transform, view.full_proj_transform)
        before = vol.weight.clone()
        chain()
        res["integrate_torch_weight_mismatches"] = int((vol.weight != before + (before > 0)).sum())      # the chain observes the same nodes
        res["integrate_torch"] = sample(chain, max(3, args.repeats // 3), 1)
    vol.reset()
    for depth, view, rgb in staged:
        vol.integrate(depth, view, rgb=rgb, sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC)
    mesh = vol.extract()
    res["extract_vertices"], res["extract_faces"] = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    res["extract_median_radius_error"] = round(float((mesh.vertices.norm(dim=1) - RADIUS).abs().median()), 6)
    res["extract_fused"] = sample(vol.extract, args.repeats, args.warmup)
    if not args.no_torch:
        chain = lambda: torch_extract_vertices(vol.tsdf, vol.weight, origin, voxel)
        res["extract_torch_vertices"] = int(chain().shape[0])
        res["extract_torch_vertex_half"] = sample(chain, max(3, args.repeats // 3), 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
