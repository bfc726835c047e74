"""utils/mcube_utils.py of the reference: marching_cubes_with_contraction, the iso-surface of any callable SDF over a lattice with an
optional inverse contraction of the vertices.

The reference evaluates the callable on the device, moves the values to the host, and runs skimage's marching cubes and trimesh's
vertex merge there.  Here the values stay where they are: they go into the tsdf plane of a gsr_mesh.TSDFVolume with weight 1 and the
surface is gsr_mesh_count / gsr_mesh_emit's (marching tetrahedra, csrc/gsr_mesh.hip), an indexed mesh without duplicate vertices from
the start.  Neither skimage nor trimesh is needed, and the resolution need not be a multiple of 512.
"""
import torch

import gsr_mesh

CHUNK = 256 ** 3          # points per call of the SDF, as in the reference


@torch.no_grad()
def marching_cubes_with_contraction(sdf, resolution=512, bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0),
                                    return_mesh=False, level=0, simplify_mesh=True, inv_contraction=None, max_range=32.0):
    """The surface sdf = level over resolution^3 nodes spanning the box, as gsr_mesh.Mesh(vertices, faces, None) on the current CUDA
    device.  `sdf` maps float32 points [m, 3] on that device to [m] values and is called on at most 256^3 points at a time.  The box
    may sit anywhere but must be a cube (one spacing for the three axes): anything else raises ValueError.  With `inv_contraction`, a
    callable on [nV, 3], the vertices are mapped through it and then clamped to [-max_range, max_range], as in the reference; without
    it they are returned as extracted.  return_mesh and simplify_mesh are accepted and ignored, as the reference ignores them; `level`
    is honoured (the reference overwrites it with 0).  Node (i, j, k) lies at bounding_box_min + spacing * (i, j, k); a node whose value
    equals `level` counts as outside (include/gsr_hip_mesh.h)."""
    lo, hi = [float(c) for c in bounding_box_min], [float(c) for c in bounding_box_max]
    n = int(resolution)
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("marching_cubes_with_contraction: the bounds have three components each")
    sides = [h - l for l, h in zip(lo, hi)]
    if not (min(sides) > 0 and max(sides) - min(sides) <= 1e-6 * max(sides)):          # (equal as float32 sees them)
        raise ValueError(f"marching_cubes_with_contraction: the box must be a cube, bounding_box_max - bounding_box_min equal and positive on "
                         f"every axis (got {sides})")
    if n < 2 or n ** 3 > gsr_mesh.MAX_NODES:
        raise ValueError(f"marching_cubes_with_contraction: resolution must be at least 2 and resolution^3 below 2^31 (got {resolution})")
    device = torch.device("cuda", torch.cuda.current_device())
    spacing = sides[0] / (n - 1)
    volume = gsr_mesh.TSDFVolume(lo, spacing, (n, n, n), device, color=False)
    volume.weight.fill_(1.0)
    values = volume.tsdf.view(-1)
    origin = torch.tensor(lo, dtype=torch.float32, device=device)
    for begin in range(0, n ** 3, CHUNK):
        node = torch.arange(begin, min(begin + CHUNK, n ** 3), device=device)
        ijk = torch.stack([node % n, (node // n) % n, node // (n * n)], dim=1)          # x fastest, as the volume's planes
        got = sdf(origin + spacing * ijk.to(torch.float32))
        values[begin:begin + len(node)] = got.reshape(-1).to(torch.float32) - float(level)
    mesh = volume.extract(min_weight=1.0)
    if inv_contraction is None:
        return mesh
    vertices = inv_contraction(mesh.vertices).to(torch.float32).clamp(-float(max_range), float(max_range))
    return gsr_mesh.Mesh(vertices, mesh.faces, None)
