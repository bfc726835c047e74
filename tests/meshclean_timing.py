"""Timing aid (not a test; needs a GPU): gsr_mesh.clean_mesh at full size against the only alternative a user of this package has.

  the mesh    the iso-surface tests/mesh_timing.py extracts (six 1920 x 1080 views of an analytic ball fused into a 512^3 volume), with
              `--floaters` synthetic components appended: fans of 1 to 100 faces each, scattered in front of, between and behind its faces
  device      clean_mesh(mesh, cluster_to_keep=1, min_triangles=50): the kernels of csrc/gsr_meshclean.hip, the 48-byte read-back and the
              allocation of the outputs, by device events, `--repeats` samples after a warm-up, median [min, max] in ms
  host        the mesh downloaded, scipy.sparse.csgraph.connected_components over its vertex graph, the same selection and compaction in
              numpy, the result uploaded: wall clock around a synchronised call, `--host-repeats` samples

Both give the same mesh (compared once, exactly).  A report, not an assertion.

    timeout -k 10 500 python tests/meshclean_timing.py [--repeats N] [--warmup W] [--size 512] [--floaters 4000] [--no-host]
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
sys.path.insert(0, ROOT)
import cameras  # noqa: E402
import gsr_synth as S  # noqa: E402
import mesh_ref as M  # noqa: E402
from mesh_timing import DEPTH_TRUNC, H, RADIUS, SDF_TRUNC, W, sample  # noqa: E402


def ball_mesh(n):
    """The mesh tests/mesh_timing.py extracts: six views round an analytic ball fused into an n^3 volume over the cameras' box."""
    import gsr_mesh
    vol = gsr_mesh.TSDFVolume((-4.0, -4.0, -4.0), 8.0 / (n - 1), (n, n, n), "cuda", color=True)
    rs = np.random.RandomState(3)
    for cam in S.circle_cameras(W, H, n=6, radius=4.0):
        depth = M.ray_depth_map(cam, (0.0, 0.0, 0.0), RADIUS, np.array([0.0, 0.0, 1.0]), 1e9)
        depth[depth > 100] = 0
        vol.integrate(torch.from_numpy(depth).cuda(), cameras.view_of(cam), rgb=torch.from_numpy(rs.rand(3, H, W).astype(np.float32)).cuda(),
                      sdf_trunc=SDF_TRUNC, depth_trunc=DEPTH_TRUNC)
    return vol.extract()


def with_floaters(mesh, count, seed=17):
    """`mesh` with `count` fans of 1..100 faces appended: their vertices behind the mesh's, their faces spliced into its face list at
    random places (a floater of a fused volume sits anywhere in the cell order)."""
    import gsr_mesh
    rs = np.random.RandomState(seed)
    nV = int(mesh.vertices.shape[0])
    sizes = rs.randint(1, 101, count)
    faces, at = [], nV
    for s in sizes:
        k = np.arange(s)
        faces.append(np.stack([np.full(s, at), at + 1 + k, at + 2 + k], 1))
        at += s + 2
    extra_f = np.concatenate(faces).astype(np.int32)
    extra_v = (rs.rand(at - nV, 3) * 8 - 4).astype(np.float32)
    extra = torch.from_numpy(extra_f).cuda()[torch.from_numpy(rs.permutation(len(extra_f))).cuda()]
    total = int(mesh.faces.shape[0]) + len(extra_f)
    slots = torch.from_numpy(np.sort(rs.choice(total, len(extra_f), replace=False))).cuda()
    body = torch.ones(total, dtype=torch.bool, device="cuda")
    body[slots] = False
    out_f = torch.empty((total, 3), dtype=torch.int32, device="cuda")
    out_f[body] = mesh.faces
    out_f[slots] = extra
    verts = torch.cat([mesh.vertices, torch.from_numpy(extra_v).cuda()])
    colors = torch.cat([mesh.colors, torch.from_numpy(rs.rand(at - nV, 3).astype(np.float32)).cuda()])
    return gsr_mesh.Mesh(verts, out_f, colors), sizes


def host_clean(mesh, cluster_to_keep, min_triangles):
    """Download, scipy's connected components, numpy selection and compaction, upload: include/gsr_hip_meshclean.h on the host (the faces
    of these meshes are all counted ones)."""
    import gsr_mesh
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    v, f, c = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.colors.cpu().numpy()
    nV = len(v)
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nV, nV)), directed=False)
    tri_comp = comp[f[:, 0]]
    sizes = np.bincount(tri_comp, minlength=comp.max() + 1)
    ranked = np.sort(sizes[sizes >= 1])[::-1]
    thr = max(int(ranked[min(cluster_to_keep, len(ranked)) - 1]), min_triangles)
    keep = sizes[tri_comp] >= thr
    used = np.zeros(nV, bool)
    used[f[keep].reshape(-1)] = True
    new_row = np.cumsum(used) - 1
    return gsr_mesh.Mesh(torch.from_numpy(v[used]).cuda(), torch.from_numpy(new_row[f[keep]].astype(np.int32)).cuda(), torch.from_numpy(c[used]).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--floaters", type=int, default=4000)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import gsr_mesh
    mesh, sizes = with_floaters(ball_mesh(args.size), args.floaters)
    res = {"what": f"clean_mesh(cluster_to_keep=1, min_triangles=50) of the {args.size}^3 six-view mesh plus {args.floaters} floaters: ms, median [min, max]",
           "repeats": args.repeats, "lib": os.environ.get("GSR_LIB", "default"),
           "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]), "floater_faces": int(sizes.sum())}
    out, info = gsr_mesh.clean_mesh(mesh, cluster_to_keep=1, min_triangles=50, return_info=True)
    res["info"] = info._asdict()
    res["device"] = sample(lambda: gsr_mesh.clean_mesh(mesh, cluster_to_keep=1, min_triangles=50), args.repeats, args.warmup)
    res["device_labels_only"] = sample(lambda: gsr_mesh.cluster_connected_triangles(mesh), args.repeats, args.warmup)
    if not args.no_host:
        ref = host_clean(mesh, 1, 50)
        res["host_equal"] = bool(torch.equal(ref.faces, out.faces) and torch.equal(ref.vertices, out.vertices) and torch.equal(ref.colors, out.colors))
        ms = []
        for _ in range(args.host_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_clean(mesh, 1, 50)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        res["host_scipy"] = {"ms_p50": round(float(np.median(ms)), 2), "ms_min": round(float(np.min(ms)), 2), "ms_max": round(float(np.max(ms)), 2),
                             "samples": args.host_repeats}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
