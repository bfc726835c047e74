"""TSDF fusion of rendered surface depth, mesh extraction and mesh clean-up on the device (include/gsr_hip_mesh.h, csrc/gsr_mesh.hip;
include/gsr_hip_meshclean.h, csrc/gsr_meshclean.hip).

A surfel model exists to yield a surface: `render()` writes `surf_depth` per view, `TSDFVolume.integrate` fuses such maps into a dense
voxel grid, `TSDFVolume.extract` pulls the iso-surface out as an indexed triangle mesh (marching tetrahedra), and `save_mesh_ply` writes
it.  Everything stays on the device; the one read-back is the 16 bytes that hold the vertex and triangle counts.  The reference took
this from open3d (ScalableTSDFVolume) on the host; utils/mesh_utils.py has its GaussianExtractor on top of this module.

`SparseTSDFVolume` is TSDFVolume in blocks of 8 x 8 x 8 nodes with storage only near the surface (include/gsr_hip_sparse.h,
csrc/gsr_sparse.hip): the same surface where the dense volume fits, and boxes of upstream's voxel size where it cannot exist.

`ContractedTSDFVolume` is the same for scenes that do not end at a box (include/gsr_hip_unbounded.h, csrc/gsr_unbounded.hip): the lattice
lies in contracted space, `extract` maps the vertices back to the world, and `color_vertices` colours them from the views afterwards.

`clean_mesh` is the step upstream runs on that mesh before writing it: the connected triangle clusters are labelled, the largest kept,
the small ones and the vertices nobody references any more dropped; `cluster_connected_triangles` gives the labels alone.  Its one
read-back is the 48 bytes of its six counts.
"""
import collections

import numpy as np
import torch

import _gsr
from _gsr import check, f32c, lib, ptr, stream_ptr

_gsr.require_entry(lib, "gsr_tsdf_integrate")

Mesh = collections.namedtuple("Mesh", "vertices faces colors")     # float32 [nV, 3], int32 [nT, 3], float32 [nV, 3] or None: device tensors
MAX_NODES = 2 ** 31 - 1
CleanInfo = collections.namedtuple("CleanInfo", "vertices faces components kept_components threshold ignored_faces")     # the six counts of gsr_mesh_clean_count


def _view_inputs(who, owner, camera, device, **maps):
    """(W, H, view, proj, {name: map}) of one view for the entries that sample it: every map that is given float32 and contiguous,
    [channels, H, W] (or [H, W] for one channel), on `device` like the two matrices.  maps: name=(tensor or None, channels); `owner` is
    what lives on `device`, for the message."""
    H, W = int(camera.image_height), int(camera.image_width)
    out = {}
    for name, (t, channels) in maps.items():
        if t is not None:
            t = f32c(t, name)
            if not (tuple(t.shape) == (channels, H, W) or (channels == 1 and tuple(t.shape) == (H, W))):
                raise ValueError(f"{who}: {name} must be [{channels}, {H}, {W}] (got {tuple(t.shape)})")
        out[name] = t
    view, proj = f32c(camera.world_view_transform, "world_view_transform"), f32c(camera.full_proj_transform, "full_proj_transform")
    for name, t in list(out.items()) + [("world_view_transform", view), ("full_proj_transform", proj)]:
        if t is not None and t.device != device:
            raise ValueError(f"{who}: {name} is on {t.device}, {owner} on {device}")
    return W, H, view, proj, out


def _iso_surface(tsdf, weight, color, dims, origin, voxel, min_weight, dev):
    """gsr_mesh_count and gsr_mesh_emit over the planes of a volume, on the current stream of `dev`: Mesh(vertices, faces, colors | None).
    Waits once, for the two counts."""
    nx, ny, nz = dims
    scratch = torch.empty(int(lib.gsr_mesh_scratch_bytes(nx, ny, nz)), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.gsr_mesh_count(ptr(tsdf), ptr(weight), nx, ny, nz, float(min_weight), ptr(scratch), scratch.numel(), ptr(counts), stream_ptr(dev)),
              "gsr_mesh_count")
        nV, nT = (int(c) for c in counts.tolist())
        verts = torch.empty((nV, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nT, 3), dtype=torch.int32, device=dev)
        colors = None if color is None else torch.empty((nV, 3), dtype=torch.float32, device=dev)
        check(lib.gsr_mesh_emit(ptr(tsdf), ptr(weight), ptr(color), nx, ny, nz, *origin, voxel, float(min_weight), ptr(scratch), ptr(verts), ptr(colors),
                                ptr(faces), nV, nT, stream_ptr(dev)), "gsr_mesh_emit")
    return Mesh(verts, faces, colors)


class TSDFVolume:
    """A dense volume of dims = (nx, ny, nz) nodes, node (i, j, k) at origin + voxel_size * (i, j, k): float32 planes tsdf [nz, ny, nx],
    weight [nz, ny, nx] and, with color=True, color [3, nz, ny, nx] on `device`, all zero when fresh."""

    def __init__(self, origin, voxel_size, dims, device, color=True):
        self.origin = tuple(float(c) for c in origin)
        self.voxel_size = float(voxel_size)
        self.dims = tuple(int(d) for d in dims)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError("TSDFVolume: origin and dims have three components")
        nx, ny, nz = self.dims
        if min(self.dims) < 2 or nx * ny * nz > MAX_NODES:
            raise ValueError(f"TSDFVolume: every dimension must be at least 2 and nx * ny * nz below 2^31 (got {self.dims})")
        if not (np.isfinite(self.voxel_size) and self.voxel_size > 0):
            raise ValueError(f"TSDFVolume: voxel_size must be positive and finite (got {voxel_size})")
        self.device = torch.device(device)
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None

    def reset(self):
        for t in (self.tsdf, self.weight, self.color):
            if t is not None:
                t.zero_()

    def integrate(self, depth, camera, rgb=None, alpha=None, alpha_min=0.5, sdf_trunc=None, depth_trunc=None):
        """Fuses one view (gsr_tsdf_integrate): depth [H, W] or [1, H, W] (render()'s surf_depth), `camera` any object render() accepts
        (world_view_transform, full_proj_transform, image_width, image_height), rgb [3, H, W] when the volume holds colour, alpha
        [H, W] or [1, H, W] to leave out pixels below alpha_min.  sdf_trunc defaults to five voxels; depth_trunc has no default.  Runs
        on the current stream; nothing is read back."""
        if depth_trunc is None:
            raise ValueError("TSDFVolume.integrate: depth_trunc is required")
        sdf_trunc = 5.0 * self.voxel_size if sdf_trunc is None else float(sdf_trunc)
        if (rgb is None) != (self.color is None):
            raise ValueError("TSDFVolume.integrate: rgb is given exactly when the volume holds colour")
        W, H, view, proj, maps = _view_inputs("TSDFVolume.integrate", "the volume", camera, self.tsdf.device, depth=(depth, 1), rgb=(rgb, 3),
                                              alpha=(alpha, 1))
        depth, rgb, alpha = maps["depth"], maps["rgb"], maps["alpha"]
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            check(lib.gsr_tsdf_integrate(ptr(self.tsdf), ptr(self.weight), ptr(self.color), nx, ny, nz, *self.origin, self.voxel_size, ptr(depth),
                                         ptr(rgb), ptr(alpha), float(alpha_min), W, H, ptr(view), ptr(proj), sdf_trunc, float(depth_trunc),
                                         stream_ptr(self.device)), "gsr_tsdf_integrate")

    def extract(self, min_weight=1.0):
        """The iso-surface tsdf = 0 over the cells whose eight nodes have weight >= min_weight, as Mesh(vertices, faces, colors) on the
        device; an empty surface gives empty tensors.  Waits once, for the two counts."""
        return _iso_surface(self.tsdf, self.weight, self.color, self.dims, self.origin, self.voxel_size, min_weight, self.device)


MAX_BLOCKS = 2 ** 31 - 1          # blocks of 8 x 8 x 8 nodes in the box of a SparseTSDFVolume
MAX_SLOTS = 2 ** 22 - 1           # slots of its pool: 512 nodes each, below 2^31 in all


def sparse_blocks(dims):
    """(gx, gy, gz) of the block grid of a SparseTSDFVolume of `dims` nodes."""
    return tuple((int(d) + 7) // 8 for d in dims)


class SparseTSDFVolume:
    """The volume of TSDFVolume (dims = (nx, ny, nz) nodes, node (i, j, k) at origin + voxel_size * (i, j, k)) stored in blocks of 8 x 8 x 8
    nodes, of which only those near the surface get storage (include/gsr_hip_sparse.h): a direct table of one int32 per block, and a pool
    of tsdf [capacity, 512], weight [capacity, 512] and, with color=True, color [capacity, 3, 512].  Use it in two phases: `touch` every
    view, `allocate` once, `integrate` every view, `extract`; the surface is then the dense volume's.  The limits are 2^31 - 1 blocks in
    the box and 2^22 - 1 allocated blocks, where the dense volume stops at 2^31 - 1 nodes."""

    def __init__(self, origin, voxel_size, dims, device, color=True):
        _gsr.require_entry(lib, "gsr_sparse_tsdf_touch")
        self.origin = tuple(float(c) for c in origin)
        self.voxel_size = float(voxel_size)
        self.dims = tuple(int(d) for d in dims)
        if len(self.origin) != 3 or len(self.dims) != 3:
            raise ValueError("SparseTSDFVolume: origin and dims have three components")
        self.grid = sparse_blocks(self.dims)
        if min(self.dims) < 2 or self.grid[0] * self.grid[1] * self.grid[2] > MAX_BLOCKS:
            raise ValueError(f"SparseTSDFVolume: every dimension must be at least 2 and the box hold fewer than 2^31 blocks of 8 x 8 x 8 nodes "
                             f"(got {self.dims})")
        if not (np.isfinite(self.voxel_size) and self.voxel_size > 0):
            raise ValueError(f"SparseTSDFVolume: voxel_size must be positive and finite (got {voxel_size})")
        self.device = torch.device(device)
        self.has_color = bool(color)
        self.table = torch.full((self.grid[0] * self.grid[1] * self.grid[2],), -1, dtype=torch.int32, device=self.device)
        self.device = self.table.device                       # ("cuda" as "cuda:0": what the views' tensors are compared with)
        self.counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._blocks = 0
        self._pool(0)

    def _pool(self, capacity):
        """A zeroed pool of `capacity` slots with the slots in use copied over."""
        old = (self.block_of_slot, self.tsdf, self.weight, self.color) if capacity else None
        dev, n = self.device, self._blocks
        self.block_of_slot = torch.zeros(capacity, dtype=torch.int32, device=dev)
        self.tsdf = torch.zeros((capacity, 512), dtype=torch.float32, device=dev)
        self.weight = torch.zeros((capacity, 512), dtype=torch.float32, device=dev)
        self.color = torch.zeros((capacity, 3, 512), dtype=torch.float32, device=dev) if self.has_color else None
        if old is not None and n:
            for new, was in zip((self.block_of_slot, self.tsdf, self.weight, self.color), old):
                if new is not None:
                    new[:n].copy_(was[:n])

    blocks = property(lambda self: self._blocks, doc="allocated blocks (slots in use)")
    capacity = property(lambda self: int(self.tsdf.shape[0]), doc="slots of the pool")

    @property
    def nbytes(self):
        """Bytes of the table and the pool."""
        return sum(t.numel() * t.element_size() for t in (self.table, self.block_of_slot, self.tsdf, self.weight, self.color) if t is not None)

    def reset(self):
        """A fresh volume: no block touched, none allocated; the pool is kept and zeroed."""
        self.table.fill_(-1)
        self.counts.zero_()
        self._blocks = 0
        for t in (self.tsdf, self.weight, self.color):
            if t is not None:
                t.zero_()

    def _truncations(self, who, sdf_trunc, depth_trunc):
        if depth_trunc is None:
            raise ValueError(f"SparseTSDFVolume.{who}: depth_trunc is required")
        return (5.0 * self.voxel_size if sdf_trunc is None else float(sdf_trunc)), float(depth_trunc)

    def touch(self, depth, camera, alpha=None, alpha_min=0.5, sdf_trunc=None, depth_trunc=None):
        """Marks the blocks this view's truncation band reaches (gsr_sparse_tsdf_touch), with a margin of one node; the arguments are
        integrate's, and must be the same for the surface to be the dense one.  Runs on the current stream; nothing is read back."""
        sdf_trunc, depth_trunc = self._truncations("touch", sdf_trunc, depth_trunc)
        W, H, view, proj, maps = _view_inputs("SparseTSDFVolume.touch", "the volume", camera, self.device, depth=(depth, 1), alpha=(alpha, 1))
        with torch.cuda.device(self.device):
            check(lib.gsr_sparse_tsdf_touch(ptr(self.table), *self.dims, *self.origin, self.voxel_size, ptr(maps["depth"]), ptr(maps["alpha"]),
                                            float(alpha_min), W, H, ptr(view), ptr(proj), sdf_trunc, depth_trunc, stream_ptr(self.device)),
                  "gsr_sparse_tsdf_touch")

    def _allocate_once(self, scratch):
        with torch.cuda.device(self.device):
            check(lib.gsr_sparse_tsdf_allocate(ptr(self.table), *self.dims, ptr(self.block_of_slot), self.capacity, ptr(self.counts), ptr(scratch),
                                               scratch.numel(), stream_ptr(self.device)), "gsr_sparse_tsdf_allocate")

    def allocate(self):
        """Gives every touched block a slot, in ascending block index behind the slots in use (gsr_sparse_tsdf_allocate), growing the pool
        when it is too small: a larger zeroed pool, the old slots copied, the entry run again (every waiting block then fits, so its
        counts are known).  Returns the number of allocated blocks.  Waits once, for the 16 bytes of the two counts."""
        scratch = torch.empty(int(lib.gsr_sparse_tsdf_allocate_scratch_bytes(*self.dims)), dtype=torch.uint8, device=self.device)
        self._allocate_once(scratch)
        allocated, wanted = (int(c) for c in self.counts.tolist())
        self._blocks = allocated
        if wanted > allocated:
            if wanted > MAX_SLOTS:
                raise ValueError(f"SparseTSDFVolume.allocate: {wanted} blocks are wanted, beyond the 2^22 - 1 of a pool (512 nodes each, below 2^31 "
                                 "nodes in all)")
            self._pool(wanted)
            self._allocate_once(scratch)
            self._blocks = wanted
        return self._blocks

    def integrate(self, depth, camera, rgb=None, alpha=None, alpha_min=0.5, sdf_trunc=None, depth_trunc=None):
        """Fuses one view into the allocated blocks (gsr_sparse_tsdf_integrate); TSDFVolume.integrate's arguments.  Runs on the current
        stream; nothing is read back."""
        sdf_trunc, depth_trunc = self._truncations("integrate", sdf_trunc, depth_trunc)
        if (rgb is None) != (self.color is None):
            raise ValueError("SparseTSDFVolume.integrate: rgb is given exactly when the volume holds colour")
        W, H, view, proj, maps = _view_inputs("SparseTSDFVolume.integrate", "the volume", camera, self.device, depth=(depth, 1), rgb=(rgb, 3),
                                              alpha=(alpha, 1))
        with torch.cuda.device(self.device):
            check(lib.gsr_sparse_tsdf_integrate(ptr(self.block_of_slot), self._blocks, self.capacity, ptr(self.tsdf), ptr(self.weight), ptr(self.color),
                                                *self.dims, *self.origin, self.voxel_size, ptr(maps["depth"]), ptr(maps["rgb"]), ptr(maps["alpha"]),
                                                float(alpha_min), W, H, ptr(view), ptr(proj), sdf_trunc, depth_trunc, stream_ptr(self.device)),
                  "gsr_sparse_tsdf_integrate")

    def extract(self, min_weight=1.0):
        """The iso-surface over the allocated blocks (gsr_sparse_mesh_count, gsr_sparse_mesh_emit) as Mesh(vertices, faces, colors) on the
        device, vertices and faces in pool order; an empty surface gives empty tensors.  Waits once, for the two counts."""
        dev, n = self.device, self._blocks
        scratch = torch.empty(int(lib.gsr_sparse_mesh_scratch_bytes(n)), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        pool = (ptr(self.table), ptr(self.block_of_slot), n, self.capacity, ptr(self.tsdf), ptr(self.weight))
        with torch.cuda.device(dev):
            check(lib.gsr_sparse_mesh_count(*pool, *self.dims, float(min_weight), ptr(scratch), scratch.numel(), ptr(counts), stream_ptr(dev)),
                  "gsr_sparse_mesh_count")
            nV, nT = (int(c) for c in counts.tolist())
            verts = torch.empty((nV, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((nT, 3), dtype=torch.int32, device=dev)
            colors = None if self.color is None else torch.empty((nV, 3), dtype=torch.float32, device=dev)
            check(lib.gsr_sparse_mesh_emit(*pool, ptr(self.color), *self.dims, *self.origin, self.voxel_size, float(min_weight), ptr(scratch),
                                           ptr(verts), ptr(colors), ptr(faces), nV, nT, stream_ptr(dev)), "gsr_sparse_mesh_emit")
        return Mesh(verts, faces, colors)

    def to_dense(self):
        """(tsdf [nz, ny, nx], weight [nz, ny, nx], color [3, nz, ny, nx] | None) as TSDFVolume lays them out, zeros where nothing is
        allocated: torch ops, for volumes below 2^31 nodes (what tests compare)."""
        nx, ny, nz = self.dims
        gx, gy, gz = self.grid
        if nx * ny * nz > MAX_NODES:
            raise ValueError(f"SparseTSDFVolume.to_dense: nx * ny * nz must be below 2^31 (got {self.dims})")
        n, b = self._blocks, self.block_of_slot[:self._blocks].long()

        def dense(pool, channels):
            full = torch.zeros((gx * gy * gz, channels, 8, 8, 8), dtype=torch.float32, device=self.device)
            full[b] = pool[:n].reshape(n, channels, 8, 8, 8)
            # [bk, bj, bi, c, lk, lj, li] -> [c, bk, lk, bj, lj, bi, li]
            full = full.reshape(gz, gy, gx, channels, 8, 8, 8).permute(3, 0, 4, 1, 5, 2, 6).reshape(channels, gz * 8, gy * 8, gx * 8)
            return full[:, :nz, :ny, :nx].contiguous()
        return dense(self.tsdf, 1)[0], dense(self.weight, 1)[0], None if self.color is None else dense(self.color, 3)


class ContractedTSDFVolume:
    """A cubic lattice of resolution^3 nodes in CONTRACTED space (include/gsr_hip_unbounded.h) about the world sphere (center, radius): node
    (i, j, k) sits at the contracted coordinate -extent + step * (i, j, k), step = 2 extent / (resolution - 1); the unit ball is the
    sphere itself and the shell 1 <= |y| < 2 holds everything beyond it.  Planes tsdf and weight, float32 [n, n, n] on `device`, both 1
    when fresh: an unseen node is free space.  The truncation is five voxels of 2 radius / resolution inside the ball and grows with
    the distance beyond it.  There are no colour planes: color_vertices colours the extracted vertices."""

    def __init__(self, center, radius, resolution, extent, device):
        self.center = tuple(float(c) for c in center)
        self.radius, self.resolution, self.extent = float(radius), int(resolution), float(extent)
        if len(self.center) != 3 or not all(np.isfinite(c) for c in self.center):
            raise ValueError(f"ContractedTSDFVolume: center has three finite components (got {center})")
        if not (np.isfinite(self.radius) and self.radius > 0):
            raise ValueError(f"ContractedTSDFVolume: radius must be positive and finite (got {radius})")
        if not 0 < self.extent <= 1.9:
            raise ValueError(f"ContractedTSDFVolume: extent must lie in (0, 1.9] (got {extent})")
        n = self.resolution
        if n < 2 or n ** 3 > MAX_NODES:
            raise ValueError(f"ContractedTSDFVolume: resolution must be at least 2 and resolution^3 below 2^31 (got {resolution})")
        self.lo, self.step, self.voxel_size = -self.extent, 2.0 * self.extent / (n - 1), 2.0 * self.radius / n
        self.device = torch.device(device)
        self.tsdf = torch.ones((n, n, n), dtype=torch.float32, device=self.device)
        self.weight = torch.ones((n, n, n), dtype=torch.float32, device=self.device)

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.fill_(1.0)

    def integrate(self, depth, camera):
        """Fuses one view (gsr_tsdf_integrate_contracted): depth [H, W] or [1, H, W] (render()'s surf_depth), `camera` any object render()
        accepts.  Runs on the current stream; nothing is read back."""
        _gsr.require_entry(lib, "gsr_tsdf_integrate_contracted")
        W, H, view, proj, maps = _view_inputs("ContractedTSDFVolume.integrate", "the volume", camera, self.tsdf.device, depth=(depth, 1))
        with torch.cuda.device(self.device):
            check(lib.gsr_tsdf_integrate_contracted(ptr(self.tsdf), ptr(self.weight), self.resolution, self.lo, self.step, *self.center, self.radius,
                                                    self.voxel_size, ptr(maps["depth"]), W, H, ptr(view), ptr(proj), stream_ptr(self.device)),
                  "gsr_tsdf_integrate_contracted")

    def extract(self, max_range=32.0):
        """The iso-surface tsdf = 0 of the lattice (gsr_mesh_count and gsr_mesh_emit with min_weight = 1: every cell), its vertices mapped
        back to the world and clamped to [-max_range, max_range] per coordinate (gsr_uncontract_points, in place): Mesh(vertices, faces,
        None) on the device.  Waits once, for the two counts."""
        _gsr.require_entry(lib, "gsr_uncontract_points")
        n, dev = self.resolution, self.device
        mesh = _iso_surface(self.tsdf, self.weight, None, (n, n, n), (self.lo,) * 3, self.step, 1.0, dev)
        with torch.cuda.device(dev):
            check(lib.gsr_uncontract_points(ptr(mesh.vertices), ptr(mesh.vertices), mesh.vertices.shape[0], *self.center, self.radius, float(max_range),
                                            stream_ptr(dev)), "gsr_uncontract_points")
        return mesh


def color_vertices(vertices, views, sdf_trunc):
    """Per-vertex colours of WORLD points [nV, 3] (gsr_points_fuse_view, one launch per view): `views` iterates (camera, depth [H, W] or
    [1, H, W], rgb [3, H, W]); a vertex gets the mean of the bilinear samples of the views that see it within sdf_trunc of their
    surface, and stays black where none does.  float32 [nV, 3] on the vertices' device; runs on the current stream, nothing is read
    back."""
    _gsr.require_entry(lib, "gsr_points_fuse_view")
    vertices = f32c(vertices, "vertices")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"color_vertices: vertices must be [nV, 3] (got {tuple(vertices.shape)})")
    dev, nV = vertices.device, int(vertices.shape[0])
    color = torch.zeros((nV, 3), dtype=torch.float32, device=dev)
    weight = torch.zeros(nV, dtype=torch.float32, device=dev)
    for camera, depth, rgb in views:
        W, H, view, proj, maps = _view_inputs("color_vertices", "the vertices", camera, dev, depth=(depth, 1), rgb=(rgb, 3))
        with torch.cuda.device(dev):
            check(lib.gsr_points_fuse_view(ptr(vertices), nV, ptr(color), ptr(weight), ptr(maps["depth"]), ptr(maps["rgb"]), W, H, ptr(view), ptr(proj),
                                           float(sdf_trunc), stream_ptr(dev)), "gsr_points_fuse_view")
    return color


def _clean_count(mesh, cluster_to_keep, min_triangles, want_labels):
    """gsr_mesh_clean_count on the current stream of the mesh's device: (faces as passed, scratch, counts [6] int64 on the device, tri_label,
    tri_size).  The entries are looked up here, not at import: everything else in this module works with a library built before them."""
    _gsr.require_entry(lib, "gsr_mesh_clean_count")
    cluster_to_keep, min_triangles = int(cluster_to_keep), int(min_triangles)
    verts, faces = mesh.vertices, mesh.faces
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"clean_mesh: vertices must be [nV, 3] and faces int32 [nT, 3] (got {tuple(verts.shape)}, {faces.dtype} {tuple(faces.shape)})")
    if faces.device != verts.device or (mesh.colors is not None and (mesh.colors.device != verts.device or mesh.colors.shape != verts.shape)):
        raise ValueError("clean_mesh: vertices, faces and colors must lie on one device, colors shaped as vertices")
    dev = verts.device
    nV, nT = int(verts.shape[0]), int(faces.shape[0])
    if nV >= 2 ** 31 or 3 * nT >= 2 ** 31:
        raise ValueError(f"clean_mesh: nV and 3 * nT must be below 2^31 (got {nV} vertices, {nT} faces)")
    faces = faces.contiguous()
    scratch = torch.empty(int(lib.gsr_mesh_clean_scratch_bytes(nV, nT)), dtype=torch.uint8, device=dev)
    counts = torch.empty(6, dtype=torch.int64, device=dev)
    tri_label = torch.empty(nT, dtype=torch.int32, device=dev) if want_labels else None
    tri_size = torch.empty(nT, dtype=torch.int32, device=dev) if want_labels else None
    with torch.cuda.device(dev):
        check(lib.gsr_mesh_clean_count(ptr(faces), nV, nT, min(cluster_to_keep, 2 ** 64 - 1), min(min_triangles, 2 ** 64 - 1), ptr(tri_label),
                                       ptr(tri_size), ptr(scratch), scratch.numel(), ptr(counts), stream_ptr(dev)), "gsr_mesh_clean_count")
    return faces, scratch, counts, tri_label, tri_size


def cluster_connected_triangles(mesh):
    """(tri_label, tri_size), int32 [nT] on the mesh's device: per face the label of its connected component (the smallest vertex index
    in it) and the number of faces in that component; a face with an index outside [0, nV) or a repeated index gets -1 and 0.  Two faces
    are connected when they share a VERTEX (open3d's function of this name asks for a shared edge; include/gsr_hip_meshclean.h).  Runs on
    the current stream; nothing is read back."""
    _, _, _, tri_label, tri_size = _clean_count(mesh, 1, 0, True)
    return tri_label, tri_size


def clean_mesh(mesh, cluster_to_keep=1000, min_triangles=50, return_info=False):
    """The mesh without its floaters (include/gsr_hip_meshclean.h): the faces of the `cluster_to_keep` largest connected components (ties
    with the last of them included, fewer components: all of them) that have at least `min_triangles` faces, in their order, and the
    vertices (and colours) those faces name, in their order, bit for bit; the faces index the new rows.  A new Mesh on the same device;
    `mesh` is not changed.  return_info=True: (Mesh, CleanInfo), the six counts.  Runs on the current stream and waits once, for the
    48 bytes of the counts; an empty mesh gives an empty Mesh without a launch."""
    _gsr.require_entry(lib, "gsr_mesh_clean_count")
    dev = mesh.vertices.device
    nV, nT = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    has_color = mesh.colors is not None
    if int(cluster_to_keep) < 1 or int(min_triangles) < 0:
        raise ValueError(f"clean_mesh: cluster_to_keep must be at least 1 and min_triangles at least 0 (got {cluster_to_keep}, {min_triangles})")
    if nV == 0 or nT == 0:
        empty = Mesh(torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                     torch.empty((0, 3), dtype=torch.float32, device=dev) if has_color else None)
        return (empty, CleanInfo(0, 0, 0, 0, 0, nT)) if return_info else empty
    verts = f32c(mesh.vertices, "vertices")
    colors = f32c(mesh.colors, "colors") if has_color else None
    faces, scratch, counts, _, _ = _clean_count(mesh, cluster_to_keep, min_triangles, False)
    info = CleanInfo(*(int(c) & (2 ** 64 - 1) for c in counts.tolist()))
    with torch.cuda.device(dev):
        verts_out = torch.empty((info.vertices, 3), dtype=torch.float32, device=dev)
        faces_out = torch.empty((info.faces, 3), dtype=torch.int32, device=dev)
        colors_out = torch.empty((info.vertices, 3), dtype=torch.float32, device=dev) if has_color else None
        check(lib.gsr_mesh_clean_emit(ptr(verts), ptr(colors), ptr(faces), nV, nT, ptr(scratch), ptr(verts_out), ptr(colors_out), ptr(faces_out),
                                      info.vertices, info.faces, stream_ptr(dev)), "gsr_mesh_clean_emit")
    out = Mesh(verts_out, faces_out, colors_out)
    return (out, info) if return_info else out


def save_mesh_ply(path, mesh):
    """Binary little-endian PLY: x y z float per vertex, with colours also red green blue uchar, quantised as
    utils.image_utils.present_bytes quantises (trunc(clamp(c, 0, 1) * 255)); faces as `list uchar int vertex_indices`."""
    verts = mesh.vertices.detach().to("cpu", torch.float32).numpy()
    faces = mesh.faces.detach().to("cpu", torch.int32).numpy()
    fields = [("xyz", "<f4", 3)]
    props = ["property float x", "property float y", "property float z"]
    if mesh.colors is not None:
        fields.append(("rgb", "u1", 3))
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    v = np.zeros(len(verts), dtype=np.dtype(fields))
    v["xyz"] = verts
    if mesh.colors is not None:
        v["rgb"] = (mesh.colors.detach().nan_to_num(0.0).clamp(0.0, 1.0) * 255.0).to(torch.uint8).cpu().numpy()
    f = np.zeros(len(faces), dtype=np.dtype([("n", "u1"), ("idx", "<i4", 3)]))
    f["n"] = 3
    f["idx"] = faces
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}"] + props + [
        f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())
