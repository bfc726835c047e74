"""utils/mesh_utils.py of the reference: GaussianExtractor, with the bounded TSDF mesh extraction its docstring promises.

The reference kept the constructor, clean() and reconstruction() and dropped the extraction together with its open3d and trimesh
imports; here the extraction is gsr_mesh.TSDFVolume (csrc/gsr_mesh.hip): the rendered maps stay on the device, the fusion and the
iso-surface run there, and the mesh comes back as device tensors (gsr_mesh.save_mesh_ply writes it).  extract_mesh_unbounded is upstream
2DGS's method of that name on gsr_mesh.ContractedTSDFVolume and gsr_mesh.color_vertices (csrc/gsr_unbounded.hip).  post_process_mesh is upstream
2DGS's clean-up of that mesh, on gsr_mesh.clean_mesh (csrc/gsr_meshclean.hip).  export_image is not provided: it needs the reference's
utils/render_utils.
"""
import math
from functools import partial

import torch

import gsr_mesh


def post_process_mesh(mesh, cluster_to_keep=1000):
    """post_process_mesh of upstream 2DGS: keeps the `cluster_to_keep` largest connected triangle clusters of `mesh`
    (gsr_mesh.Mesh, device tensors) and none below 50 triangles, drops the vertices no kept face names, and prints upstream's two lines.
    The mesh stays on the device (gsr_mesh.clean_mesh; clusters are joined over shared vertices, and a `cluster_to_keep` beyond the number
    of clusters keeps them all where upstream raises)."""
    out = gsr_mesh.clean_mesh(mesh, cluster_to_keep=cluster_to_keep, min_triangles=50)
    print("num vertices raw {}".format(len(mesh.vertices)))
    print("num vertices post {}".format(len(out.vertices)))
    return out


class GaussianExtractor:
    """GaussianExtractor(gaussians, render, pipe, bg_color=None) of the reference: renders a model from a stack of cameras and turns
    the rendered surface depth into a mesh.

        extractor = GaussianExtractor(gaussians, render, pipe)
        extractor.reconstruction(cameras)
        mesh = extractor.extract_mesh_bounded(voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3)

    `render` is gaussian_renderer.render (or a function with its signature); the background defaults to black and lives on the
    current CUDA device, as in the reference."""

    def __init__(self, gaussians, render, pipe, bg_color=None):
        self.gaussians = gaussians
        background = torch.tensor([0, 0, 0] if bg_color is None else bg_color, dtype=torch.float32, device="cuda")
        self.render = partial(render, pipe=pipe, bg_color=background)
        self.clean()

    def clean(self):
        """Drops everything the last reconstruction() kept."""
        self.viewpoint_stack = []
        self.rgbmaps, self.depthmaps, self.alphamaps, self.normals, self.depth_normals = [], [], [], [], []

    @torch.no_grad()
    def reconstruction(self, viewpoint_stack):
        """Renders every camera of `viewpoint_stack` and keeps, per view and ON THE DEVICE: `render` (rgbmaps), `surf_depth` (depthmaps),
        `rend_alpha` (alphamaps) and `rend_normal` normalised over its channels (normals).  (The reference moves the colour to the host
        and keeps nothing else but the normals; its extraction, which would have read the rest, is gone.)"""
        self.clean()
        self.viewpoint_stack = viewpoint_stack
        for cam in viewpoint_stack:
            pkg = self.render(cam, self.gaussians)
            self.rgbmaps.append(pkg["render"])
            self.depthmaps.append(pkg["surf_depth"])
            self.alphamaps.append(pkg["rend_alpha"])
            self.normals.append(torch.nn.functional.normalize(pkg["rend_normal"], dim=0))

    def camera_bounds(self):
        """(centre, radius) of the sphere about the mean of the camera centres that holds them all."""
        if not self.viewpoint_stack:
            raise ValueError("GaussianExtractor: reconstruction() has seen no cameras")
        centres = torch.stack([c.camera_center.detach().reshape(3).double().cpu() for c in self.viewpoint_stack])
        centre = centres.mean(dim=0)
        return centre, float((centres - centre).norm(dim=1).max())

    @torch.no_grad()
    def extract_mesh_bounded(self, voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3, mask_backgrond=True, bounds=None, sparse=False):
        """The bounded TSDF extraction upstream 2DGS calls by this name (the `mask_backgrond` spelling is upstream's): every kept view
        is fused into one dense volume of `voxel_size` nodes over `bounds` = ((xmin, ymin, zmin), (xmax, ymax, zmax)), truncated at
        `sdf_trunc` and ignoring depths beyond `depth_trunc`; with mask_backgrond, pixels whose rendered alpha is below 0.5 are left
        out.  bounds=None: the box around the sphere about the mean camera centre that holds every camera centre.  Returns
        gsr_mesh.Mesh(vertices, faces, colors) on the device.  A box that needs 2^31 nodes or more: ValueError.
        sparse=True: the volume is a gsr_mesh.SparseTSDFVolume, which stores the blocks of 8 x 8 x 8 nodes near the surface only, as
        upstream's ScalableTSDFVolume does: every view is touched, the blocks are allocated once, every view is fused, and the surface
        is the dense volume's (its vertices and faces come in pool order).  Its limits are 2^31 - 1 blocks in the box and 2^22 - 1
        allocated blocks; beyond them: ValueError."""
        if not self.depthmaps:
            raise ValueError("GaussianExtractor.extract_mesh_bounded: call reconstruction() first")
        if bounds is None:
            centre, radius = self.camera_bounds()
            lo, hi = [float(c) - radius for c in centre], [float(c) + radius for c in centre]
        else:
            lo, hi = [float(c) for c in bounds[0]], [float(c) for c in bounds[1]]
        voxel_size = float(voxel_size)
        if not voxel_size > 0:
            raise ValueError(f"extract_mesh_bounded: voxel_size must be positive (got {voxel_size})")
        dims = [max(2, int(math.ceil((h - l) / voxel_size)) + 1) for l, h in zip(lo, hi)]
        nodes = dims[0] * dims[1] * dims[2]
        views = list(zip(self.viewpoint_stack, self.depthmaps, self.rgbmaps, self.alphamaps))
        mask = dict(alpha_min=0.5, sdf_trunc=sdf_trunc, depth_trunc=depth_trunc)
        if sparse:
            gx, gy, gz = gsr_mesh.sparse_blocks(dims)
            if gx * gy * gz > gsr_mesh.MAX_BLOCKS:
                raise ValueError(f"extract_mesh_bounded: a volume of {dims[0]} x {dims[1]} x {dims[2]} nodes has {gx * gy * gz} blocks of 8 x 8 x 8 "
                                 "nodes, beyond the 2^31 - 1 of a sparse volume; pass a larger voxel_size or smaller bounds")
            volume = gsr_mesh.SparseTSDFVolume(lo, voxel_size, dims, self.depthmaps[0].device, color=True)
            for cam, depth, rgb, alpha in views:
                volume.touch(depth, cam, alpha=alpha if mask_backgrond else None, **mask)
            volume.allocate()            # (a ValueError beyond 2^22 - 1 allocated blocks)
            for cam, depth, rgb, alpha in views:
                volume.integrate(depth, cam, rgb=rgb, alpha=alpha if mask_backgrond else None, **mask)
            return volume.extract()
        if nodes > gsr_mesh.MAX_NODES:
            # the edge count per axis scales with 1 / voxel_size: the smallest voxel whose node count fits, with a little room for the ceil
            fit = voxel_size * (nodes / gsr_mesh.MAX_NODES) ** (1.0 / 3.0) * 1.01
            raise ValueError(f"extract_mesh_bounded: a volume of {dims[0]} x {dims[1]} x {dims[2]} = {nodes} nodes is beyond the 2^31 - 1 of a "
                             f"dense volume; voxel_size >= {fit:.6g} fits these bounds (or pass smaller bounds, or sparse=True)")
        volume = gsr_mesh.TSDFVolume(lo, voxel_size, dims, self.depthmaps[0].device, color=True)
        for cam, depth, rgb, alpha in views:
            volume.integrate(depth, cam, rgb=rgb, alpha=alpha if mask_backgrond else None, **mask)
        return volume.extract()

    def contracted_extent(self, centre, radius):
        """Half the side of the lattice extract_mesh_unbounded lays out, in contracted units: the 0.95 quantile (linear interpolation
        between order statistics) of the model's contracted norms about (centre, radius), a norm m counting as m below 1 and as
        2 - 1 / m beyond, plus 0.01 and at most 1.9.  Torch ops and one host read."""
        xyz = self.gaussians.get_xyz.detach().to(torch.float32)
        m = ((xyz - torch.as_tensor([float(c) for c in centre], dtype=torch.float32, device=xyz.device)) / float(radius)).norm(dim=1)
        if m.numel() == 0:
            raise ValueError("GaussianExtractor: the model has no Gaussians")
        g = torch.where(m < 1, m, 2 - 1 / m).sort().values               # (torch.quantile stops at 2^24 elements)
        at = 0.95 * (g.numel() - 1)
        below = int(math.floor(at))
        a, b = g[[below, min(below + 1, g.numel() - 1)]].tolist()
        return min(a + (b - a) * (at - below) + 0.01, 1.9)

    @torch.no_grad()
    def extract_mesh_unbounded(self, resolution=1024):
        """The unbounded TSDF extraction upstream 2DGS calls by this name: every kept view is fused into a lattice of resolution^3 nodes in
        contracted space (gsr_mesh.ContractedTSDFVolume: the sphere of camera_bounds() is the unit ball, everything beyond it is folded
        into the shell up to 2), the iso-surface is extracted and mapped back to the world, and the vertices are coloured from the views
        with the truncation of five voxels.  The lattice reaches as far as contracted_extent() says.  Returns gsr_mesh.Mesh(vertices,
        faces, colors) on the device.  include/gsr_hip_unbounded.h states where this differs from upstream."""
        if not self.depthmaps:
            raise ValueError("GaussianExtractor.extract_mesh_unbounded: call reconstruction() first")
        centre, radius = self.camera_bounds()
        volume = gsr_mesh.ContractedTSDFVolume(centre, radius, resolution, self.contracted_extent(centre, radius), self.depthmaps[0].device)
        for cam, depth in zip(self.viewpoint_stack, self.depthmaps):
            volume.integrate(depth, cam)
        mesh = volume.extract()
        colors = gsr_mesh.color_vertices(mesh.vertices, zip(self.viewpoint_stack, self.depthmaps, self.rgbmaps), 5.0 * volume.voxel_size)
        return gsr_mesh.Mesh(mesh.vertices, mesh.faces, colors)
