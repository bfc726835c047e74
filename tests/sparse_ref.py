"""float64 numpy restatement of include/gsr_hip_sparse.h (test infrastructure only), on top of tests/mesh_ref.py, whose tables and per-node
rule it uses: which blocks a view touches, the allocation of slots, the fusion into the pool and the iso-surface in pool order.

  grid(dims), block_index / block_coords       the block grid and its linear index
  touch(dims, origin, voxel, view...)          -> (sure, possible): sorted block indices.  `sure` comes from the band nodes whose every
                                               decision is stable; `possible` from the nodes that are band nodes under some admissible
                                               decision: mesh_ref.integrate's instabilities (a pixel coordinate within 1e-3 of a
                                               half-integer, z, p.w or depth_trunc - d within 1e-5 of zero, sdf within 1e-4 sdf_trunc of
                                               -sdf_trunc) and sdf within 1e-4 sdf_trunc of +sdf_trunc.  A node near a pixel tie is
                                               evaluated under each candidate pixel, not simply counted as possible.
  allocate(table, block_of_slot, capacity, counts)   slots in ascending block index; returns the new counts
  Volume                                       table, block_of_slot and float64 pool planes; touch / allocate / integrate / to_dense
  extract(vol, min_weight)                     (verts, colors, faces, keys, face_cells) in pool order; keys and face_cells carry the
                                               dense node and cell indices, so a dense extraction can be permuted onto it
  to_pool_order(...)                           mesh_ref.extract's result permuted into pool order
"""
import itertools

import numpy as np

import mesh_ref as M

B = 8                      # nodes per block and axis
UNTOUCHED, WAITING = -1, -2


def grid(dims):
    return tuple((d + B - 1) // B for d in dims)


def block_index(bi, bj, bk, dims):
    gx, gy, _ = grid(dims)
    return (bk * gy + bj) * gx + bi


def block_coords(b, dims):
    gx, gy, _ = grid(dims)
    return b % gx, (b // gx) % gy, b // (gx * gy)


def blocks_near(nodes, dims):
    """Sorted linear indices of the blocks that hold an existing node within one node (Chebyshev) of a node of the mask [nz, ny, nx]."""
    nx, ny, nz = dims
    near = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    for dz, dy, dx in itertools.product((0, 1, 2), repeat=3):
        near[dz:dz + nz, dy:dy + ny, dx:dx + nx] |= nodes
    k, j, i = np.nonzero(near[1:-1, 1:-1, 1:-1])
    return np.unique(block_index(i // B, j // B, k // B, dims))


def touch(dims, origin, voxel, depth, alpha, alpha_min, viewmatrix, projmatrix, sdf_trunc, depth_trunc):
    """(sure, possible) of one view: steps 1-3 of mesh_ref.integrate in float64 on the float32 inputs, then the band test."""
    nx, ny, nz = dims
    H, W = depth.shape
    o, h = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(voxel))
    X, Y, Z = o[0] + h * np.arange(nx), o[1] + h * np.arange(ny), o[2] + h * np.arange(nz)
    V, P = np.asarray(viewmatrix, np.float32).astype(np.float64).reshape(-1), np.asarray(projmatrix, np.float32).astype(np.float64).reshape(-1)
    T, depth_trunc, alpha_min = float(np.float32(sdf_trunc)), float(np.float32(depth_trunc)), float(np.float32(alpha_min))
    depth64 = depth.astype(np.float64)
    alpha64 = None if alpha is None else alpha.astype(np.float64)
    dot = lambda cx, cy, cz, c0: (cx * X)[None, None, :] + (cy * Y)[None, :, None] + (cz * Z + c0)[:, None, None]
    z, pw = dot(V[2], V[6], V[10], V[14]), dot(P[3], P[7], P[11], P[15])
    front, front_unstable = (z > 0) & (pw > 0), (np.abs(z) < 1e-5) | (np.abs(pw) < 1e-5)
    with np.errstate(all="ignore"):
        px = ((dot(P[0], P[4], P[8], P[12]) / pw + 1.0) * W - 1.0) / 2.0
        py = ((dot(P[1], P[5], P[9], P[13]) / pw + 1.0) * H - 1.0) / 2.0
    near_tie = lambda q: np.abs(q - np.floor(q) - 0.5) < 1e-3
    tie_x, tie_y = near_tie(px) & np.isfinite(px), near_tie(py) & np.isfinite(py)
    sure = np.zeros((nz, ny, nx), bool)
    possible = np.zeros((nz, ny, nx), bool)
    # candidate pixels: rint, and at a near tie the pixel on either side of the half-integer
    for cu, cv in itertools.product((0, 1, 2), repeat=2):
        with np.errstate(invalid="ignore"):
            u = np.rint(px) if cu == 0 else np.floor(px) + (cu - 1)
            v = np.rint(py) if cv == 0 else np.floor(py) + (cv - 1)
            use = (np.ones_like(tie_x) if cu == 0 else tie_x) & (np.ones_like(tie_y) if cv == 0 else tie_y)
            use &= (u >= 0) & (u < W) & (v >= 0) & (v < H)               # (NaN: not used)
        at = np.nonzero(use)
        ui, vi = u[at].astype(np.int64), v[at].astype(np.int64)
        d = depth64[vi, ui]
        with np.errstate(invalid="ignore"):
            seen = (d > 0) & (d <= depth_trunc)
            seen_unstable = np.abs(depth_trunc - d) < 1e-5
            masked = np.zeros(len(d), bool) if alpha64 is None else ~(alpha64[vi, ui] >= alpha_min)
            sdf = d - z[at]
            band = (sdf >= -T) & (sdf < T)
            band_unstable = (np.abs(sdf + T) < 1e-4 * T) | (np.abs(sdf - T) < 1e-4 * T)
        f, fu = front[at], front_unstable[at]
        possible[at] |= (f | fu) & (seen | seen_unstable) & ~masked & (band | band_unstable)
        if cu == 0 and cv == 0:
            stable = ~fu & ~seen_unstable & ~band_unstable & ~tie_x[at] & ~tie_y[at]
            sure[at] |= f & seen & ~masked & band & stable
    assert not (sure & ~possible).any()
    return blocks_near(sure, dims), blocks_near(possible, dims)


def allocate(table, block_of_slot, capacity, counts):
    """include/gsr_hip_sparse.h, gsr_sparse_tsdf_allocate: `table` and `block_of_slot` (length >= capacity) are updated in place; returns
    the new (allocated, wanted)."""
    slot = int(counts[0])
    waiting = np.nonzero(table == WAITING)[0]
    for b in waiting:
        if slot < capacity:
            table[b] = slot
            block_of_slot[slot] = b
        slot += 1
    return min(slot, capacity), slot


class Volume:
    """A sparse volume with float64 pool planes (the device's are float32)."""

    def __init__(self, dims, origin, voxel, color=True):
        self.dims, self.origin, self.voxel, self.has_color = tuple(dims), origin, voxel, color
        gx, gy, gz = grid(dims)
        self.table = np.full(gx * gy * gz, UNTOUCHED, np.int32)
        self.counts = (0, 0)
        self._pool(0)

    def _pool(self, capacity):
        n = self.counts[0]
        old = (self.block_of_slot, self.tsdf, self.weight, self.color) if capacity else None
        self.block_of_slot = np.zeros(capacity, np.int32)
        self.tsdf, self.weight = np.zeros((capacity, 512)), np.zeros((capacity, 512))
        self.color = np.zeros((capacity, 3, 512)) if self.has_color else None
        if old is not None:
            for new, was in zip((self.block_of_slot, self.tsdf, self.weight, self.color), old):
                if new is not None:
                    new[:n] = was[:n]

    blocks = property(lambda self: self.counts[0])

    def touch(self, vw, alpha_min, sdf_trunc, depth_trunc, alpha=True, which="possible"):
        sure, possible = touch(self.dims, self.origin, self.voxel, vw["depth"], vw["alpha"] if alpha else None, alpha_min, vw["cam"]["viewmatrix"],
                               vw["cam"]["projmatrix"], sdf_trunc, depth_trunc)
        hit = sure if which == "sure" else possible
        self.table[hit[self.table[hit] == UNTOUCHED]] = WAITING
        return sure, possible

    def allocate(self):
        self.counts = allocate(self.table, self.block_of_slot, len(self.block_of_slot), self.counts)
        if self.counts[1] > self.counts[0]:
            self._pool(self.counts[1])
            self.counts = allocate(self.table, self.block_of_slot, len(self.block_of_slot), self.counts)
        return self.counts[0]

    def _index(self):
        """(slot [nz, ny, nx] or -1, local [nz, ny, nx]) of every node of the box."""
        nx, ny, nz = self.dims
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        slot = self.table[block_index(i // B, j // B, k // B, self.dims)]
        slot = np.where((slot >= 0) & (slot < self.counts[0]), slot, -1)
        return slot, ((k % B) * B + j % B) * B + i % B

    def to_dense(self):
        """(tsdf, weight, color | None, allocated) as dense float64 planes [nz, ny, nx], zeros where nothing is allocated."""
        slot, local = self._index()
        has = slot >= 0
        s = np.maximum(slot, 0)
        if len(self.tsdf) == 0:
            zero = np.zeros(has.shape)
            return zero, zero.copy(), np.zeros((3,) + has.shape) if self.has_color else None, has
        pick = lambda plane: np.where(has, plane[s, local], 0.0)
        color = np.stack([np.where(has, self.color[s, c, local], 0.0) for c in range(3)]) if self.has_color else None
        return pick(self.tsdf), pick(self.weight), color, has

    def integrate(self, vw, alpha_min, sdf_trunc, depth_trunc, color=True, alpha=True):
        """One view into the allocated blocks: mesh_ref.integrate on the dense planes, of which the allocated nodes are taken back.
        Returns (written, unstable, allocated), dense masks; `written` only counts allocated nodes."""
        tsdf, weight, col, has = self.to_dense()
        dense = M.Volume(self.dims, self.origin, self.voxel, color=self.has_color)
        dense.tsdf, dense.weight, dense.color = tsdf, weight, col
        written, unstable = M.integrate(dense, vw["depth"], vw["rgb"] if color else None, vw["alpha"] if alpha else None, alpha_min,
                                        vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"], sdf_trunc, depth_trunc)
        slot, local = self._index()
        s, l = slot[has], local[has]
        self.tsdf[s, l], self.weight[s, l] = dense.tsdf[has], dense.weight[has]
        if self.has_color:
            for c in range(3):
                self.color[s, c, l] = dense.color[c][has]
        return written & has, unstable, has


def extract(table, block_of_slot, n_slots, tsdf, weight, color, dims, origin, voxel, min_weight=1.0):
    """The iso-surface over the pool (include/gsr_hip_sparse.h) with mesh_ref's tables: tsdf, weight [capacity, 512] and color
    [capacity, 3, 512] | None as float32.  Returns (verts f64 [nV, 3], colors | None, faces int32 [nT, 3], keys [(dense node linear index,
    direction)] per vertex, face_cells: the dense cell linear index of every face, ends: mesh_ref.Ends), vertices ascending in (pool node,
    direction), faces in (pool cell, tetrahedron, triangle)."""
    nx, ny, nz = dims
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    o = np.asarray(origin, np.float32).astype(np.float64)
    h = float(np.float32(voxel))

    def pool_node(i, j, k):
        """Pool index of node (i, j, k), or -1 where it does not exist or has no storage."""
        if not (0 <= i < nx and 0 <= j < ny and 0 <= k < nz):
            return -1
        s = table[block_index(i // B, j // B, k // B, dims)]
        return -1 if s < 0 or s >= n_slots else s * 512 + ((k % B) * B + j % B) * B + i % B

    flat_t, flat_w = tsdf.reshape(-1), weight.reshape(-1)

    def valid(p):
        with np.errstate(invalid="ignore"):
            return p >= 0 and bool(flat_w[p] >= np.float32(min_weight))

    def inside(p):
        with np.errstate(invalid="ignore"):
            return bool(flat_t[p] < np.float32(0))

    cell_cache = {}

    def cell_ok(i, j, k):
        key = (i, j, k)
        if key not in cell_cache:
            cell_cache[key] = (0 <= i < nx - 1 and 0 <= j < ny - 1 and 0 <= k < nz - 1 and
                               all(valid(pool_node(i + dx, j + dy, k + dz)) for dz, dy, dx in itertools.product((0, 1), repeat=3)))
        return cell_cache[key]

    def nodes_in_pool_order():
        for s in range(n_slots):
            bi, bj, bk = block_coords(int(block_of_slot[s]), dims)
            for lk, lj, li in itertools.product(range(B), repeat=3):
                i, j, k = bi * B + li, bj * B + lj, bk * B + lk
                if i < nx and j < ny and k < nz:
                    yield s * 512 + (lk * B + lj) * B + li, i, j, k

    index, verts, cols, keys, end_a, end_b, end_ca, end_cb = {}, [], [], [], [], [], [], []
    col_of = lambda p: np.array([color[p // 512, c, p % 512] for c in range(3)], np.float64)
    for p, i, j, k in nodes_in_pool_order():
        if not valid(p):
            continue
        for e, (dx, dy, dz) in enumerate(M.DIRECTIONS):
            q = pool_node(i + dx, j + dy, k + dz)
            if not valid(q) or inside(p) == inside(q):
                continue
            if not any(cell_ok(cx, cy, cz) for cx in ((i,) if dx else (i - 1, i)) for cy in ((j,) if dy else (j - 1, j))
                       for cz in ((k,) if dz else (k - 1, k))):
                continue
            ta, tb = float(flat_t[p]), float(flat_t[q])
            f = ta / (ta - tb)
            a = o + h * np.array([i, j, k], np.float64)
            b = o + h * np.array([i + dx, j + dy, k + dz], np.float64)
            index[(p, e)] = len(verts)
            keys.append(((k * ny + j) * nx + i, e))
            verts.append(a + (b - a) * f)
            end_a.append(a)
            end_b.append(b)
            if color is not None:
                ca, cb = col_of(p), col_of(q)
                cols.append(ca + (cb - ca) * f)
                end_ca.append(ca)
                end_cb.append(cb)
    faces, face_cells = [], []
    for p, i, j, k in nodes_in_pool_order():
        if not cell_ok(i, j, k):
            continue
        for t in range(6):
            c = M.tet_corners(t)
            corner = [pool_node(i + c[v][0], j + c[v][1], k + c[v][2]) for v in range(4)]
            mask = sum(1 << v for v in range(4) if inside(corner[v]))
            for tri in M.TRIANGLES[mask]:
                ids = [index[(corner[lo], M.DIRECTIONS.index(tuple(c[hi][x] - c[lo][x] for x in range(3))))] for lo, hi in tri]
                if not M.tet_positive(t):
                    ids[1], ids[2] = ids[2], ids[1]
                faces.append(ids)
                face_cells.append((k * (ny - 1) + j) * (nx - 1) + i)
    rows = lambda x: np.array(x, np.float64).reshape(-1, 3)
    ends = M.Ends(rows(end_a), rows(end_b), None if color is None else rows(end_ca), None if color is None else rows(end_cb))
    return (rows(verts), None if color is None else rows(cols), np.array(faces, np.int32).reshape(-1, 3), keys, np.array(face_cells, np.int64), ends)


def extract_volume(vol, min_weight=1.0):
    """extract() of a Volume, its planes rounded to float32 as the device's are."""
    f32 = lambda a: None if a is None else a.astype(np.float32)
    return extract(vol.table, vol.block_of_slot, vol.counts[0], f32(vol.tsdf), f32(vol.weight), f32(vol.color), vol.dims, vol.origin, vol.voxel,
                   min_weight)


def dense_keys(tsdf, weight, min_weight=1.0):
    """[(node linear index, direction)] of mesh_ref.extract's vertices, in its order (ascending), from whole-array arithmetic."""
    valid, inside, ok = M._classes(tsdf, weight, min_weight)
    nz, ny, nx = inside.shape
    cells = np.zeros((nz + 1, ny + 1, nx + 1), bool)
    cells[1:-1, 1:-1, 1:-1] = ok
    out = []
    for e, (dx, dy, dz) in enumerate(M.DIRECTIONS):
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        held = np.zeros(inside[lo].shape, bool)
        for oz, oy, ox in itertools.product(((1,) if dz else (0, 1)), ((1,) if dy else (0, 1)), ((1,) if dx else (0, 1))):
            held |= cells[oz:oz + nz - dz, oy:oy + ny - dy, ox:ox + nx - dx]
        k, j, i = np.nonzero(valid[lo] & valid[hi] & (inside[lo] != inside[hi]) & held)
        out += [(int(n), e) for n in (k * ny + j) * nx + i]
    return sorted(out)


def to_pool_order(dense_mesh, dense_vertex_keys, keys, face_cells):
    """mesh_ref.extract's (V, C, F) of the same planes, its vertices keyed by `dense_vertex_keys`, permuted into the pool order that
    extract() reports through `keys` and `face_cells`: (V, C, F) to compare with extract()'s, row by row."""
    V, C, F = dense_mesh
    assert sorted(keys) == list(dense_vertex_keys), "the two extractions do not have the same vertices"
    rank = {key: n for n, key in enumerate(dense_vertex_keys)}
    to_dense = np.array([rank[key] for key in keys], np.int64).reshape(-1)             # pool vertex -> dense vertex
    to_pool = np.empty(len(keys), np.int64)
    to_pool[to_dense] = np.arange(len(keys))
    # the dense faces ascend in (cell, tetrahedron, triangle): a stable sort of the pool's faces by dense cell index gives that order
    order = np.argsort(face_cells, kind="stable")
    assert len(order) == len(F)
    Fp = np.empty_like(F)
    Fp[order] = to_pool[F.astype(np.int64)].astype(np.int32) if len(F) else F
    return V[to_dense], None if C is None else C[to_dense], Fp
