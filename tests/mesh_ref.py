"""float64 numpy restatement of include/gsr_hip_mesh.h (test infrastructure only): TSDF integration of one view, and the marching-tetrahedra
iso-surface on the Kuhn split.  Inputs are the float32-rounded arrays the device gets; every decision (skip rules, rint's ties to even,
`inside`, `valid`, the orders of vertices and triangles, the split of a quad) follows the header, the arithmetic is float64.

  integrate(vol, view)          -> (written [nz,ny,nx] bool, unstable [nz,ny,nx] bool); vol's planes are updated in place
  extract(tsdf, weight, ...)    -> (verts [nV,3] f64, colors [nV,3] f64 | None, faces [nT,3] int32[, Ends: the end nodes of every vertex's edge])
  extract_bounds(ends, voxel)   the bound on |device - extract()| per vertex and component that follows from the kernel's arithmetic
  TRIANGLES                     the 16-case table of a positively oriented tetrahedron, generated from the header's rule
  topology(faces, nV)           edge statistics of an indexed mesh, for the known-answer tests
  sphere_grid / torus_grid      the analytic grids of tests/test_mesh_ref.py and tests/test_gpu_mesh.py
  random_lattice / config_lattice / stacked + stacked_mesh / long_column      grids without structure: random signs, exact zeros, scattered
                                invalid nodes; the 256 corner configurations once each; lattices stacked along z, their mesh composed
  coverage / held_classes       what a grid reaches: (tetrahedron, mask) pairs, corner configurations, edges held by none, some or all cells
  integrate_fixture()           the volume, cameras and depth maps of the integrate tests
"""
import collections
import itertools
import math

import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))       # lattice edge directions 0..6, (x, y, z)
TETS = ((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1))                                         # (a, b) of tetrahedra 0..5
Ends = collections.namedtuple("Ends", "a b ca cb")


def _even(perm):
    perm, swaps = list(perm), 0
    for i in range(len(perm)):
        while perm[i] != i:
            j = perm[i]
            perm[i], perm[j] = perm[j], perm[i]
            swaps += 1
    return swaps % 2 == 0


def _edge(i, j):
    return (min(i, j), max(i, j))


def _table():
    """{inside mask over (p0..p3): [triangles as three (lo, hi) local edges]} for a positively oriented tetrahedron."""
    table = {0: [], 15: []}
    for k in range(4):
        rest = [v for v in range(4) if v != k]
        i, j, l = next(p for p in itertools.permutations(rest) if _even((k,) + p) and p[0] == rest[0])
        table[1 << k] = [[_edge(k, i), _edge(k, j), _edge(k, l)]]
        table[15 ^ (1 << k)] = [[_edge(k, i), _edge(k, l), _edge(k, j)]]
    for a, b in itertools.combinations(range(4), 2):
        c, d = [v for v in range(4) if v not in (a, b)]
        if not _even((a, b, c, d)):
            c, d = d, c
        ac, ad, bd, bc = _edge(a, c), _edge(a, d), _edge(b, d), _edge(b, c)
        table[(1 << a) | (1 << b)] = [[ac, ad, bd], [ac, bd, bc]]
    return table


TRIANGLES = _table()


def tet_corners(t):
    """Offsets (x, y, z) of p0..p3 of tetrahedron t from the cell's low corner."""
    a, b = TETS[t]
    p1 = [0, 0, 0]
    p1[a] = 1
    p2 = list(p1)
    p2[b] = 1
    return ((0, 0, 0), tuple(p1), tuple(p2), (1, 1, 1))


def tet_positive(t):
    p = np.array(tet_corners(t), dtype=np.float64)
    return np.linalg.det(np.stack([p[1] - p[0], p[2] - p[0], p[3] - p[0]], 1)) > 0


# ------------------------------------------------------------------------------------------------- extraction
def extract(tsdf, weight, color, origin, voxel, min_weight=1.0, ends=False):
    """tsdf, weight [nz, ny, nx] float32, color [3, nz, ny, nx] float32 or None.  ends=True: a fourth result, Ends(a, b, ca, cb), the
    positions [nV, 3] and colours [nV, 3] | None of the two end nodes of each vertex's lattice edge (what extract_bounds() is made of)."""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        valid = weight >= np.float32(min_weight)
        inside = tsdf < np.float32(0)
    cell_ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        cell_ok &= valid[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    t64 = tsdf.astype(np.float64)
    o = np.asarray(origin, np.float32).astype(np.float64)
    h = float(np.float32(voxel))
    index = {}                     # (node linear index, direction) -> vertex index
    verts, cols, end_a, end_b, end_ca, end_cb = [], [], [], [], [], []
    for k, j, i in itertools.product(range(nz), range(ny), range(nx)):
        for e, (dx, dy, dz) in enumerate(DIRECTIONS):
            i2, j2, k2 = i + dx, j + dy, k + dz
            if i2 >= nx or j2 >= ny or k2 >= nz:
                continue
            if not (valid[k, j, i] and valid[k2, j2, i2]) or inside[k, j, i] == inside[k2, j2, i2]:
                continue
            held = False
            for cx in ((i,) if dx else (i - 1, i)):
                for cy in ((j,) if dy else (j - 1, j)):
                    for cz in ((k,) if dz else (k - 1, k)):
                        if 0 <= cx < nx - 1 and 0 <= cy < ny - 1 and 0 <= cz < nz - 1 and cell_ok[cz, cy, cx]:
                            held = True
            if not held:
                continue
            ta, tb = t64[k, j, i], t64[k2, j2, i2]
            f = ta / (ta - tb)
            a = o + h * np.array([i, j, k], np.float64)
            b = o + h * np.array([i2, j2, k2], np.float64)
            index[((k * ny + j) * nx + i, e)] = len(verts)
            verts.append(a + (b - a) * f)
            end_a.append(a)
            end_b.append(b)
            if color is not None:
                ca, cb = color[:, k, j, i].astype(np.float64), color[:, k2, j2, i2].astype(np.float64)
                cols.append(ca + (cb - ca) * f)
                end_ca.append(ca)
                end_cb.append(cb)
    faces = []
    for k, j, i in itertools.product(range(nz - 1), range(ny - 1), range(nx - 1)):
        if not cell_ok[k, j, i]:
            continue
        for t in range(6):
            p = tet_corners(t)
            mask = sum(1 << v for v in range(4) if inside[k + p[v][2], j + p[v][1], i + p[v][0]])
            for tri in TRIANGLES[mask]:
                ids = []
                for lo, hi in tri:
                    n = ((k + p[lo][2]) * ny + j + p[lo][1]) * nx + i + p[lo][0]
                    d = tuple(p[hi][c] - p[lo][c] for c in range(3))
                    ids.append(index[(n, DIRECTIONS.index(d))])
                if not tet_positive(t):
                    ids[1], ids[2] = ids[2], ids[1]
                faces.append(ids)
    V = np.array(verts, np.float64).reshape(-1, 3)
    C = None if color is None else np.array(cols, np.float64).reshape(-1, 3)
    F = np.array(faces, np.int32).reshape(-1, 3)
    if not ends:
        return V, C, F
    rows = lambda x: np.array(x, np.float64).reshape(-1, 3)
    return V, C, F, Ends(rows(end_a), rows(end_b), None if color is None else rows(end_ca), None if color is None else rows(end_cb))


def extract_vertices(tsdf, weight, origin, voxel, min_weight=1.0):
    """The vertex positions of extract() alone, [nV, 3] float64 grouped by direction (not in the mesh's order): whole-array arithmetic,
    for volumes too large for extract()'s loops.  `origin` is taken as given (float64), voxel rounded to float32."""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        valid = weight >= np.float32(min_weight)
        inside = tsdf < np.float32(0)
    cells = np.zeros((nz + 1, ny + 1, nx + 1), bool)          # cell c at index c + 1, no cell beyond the borders
    ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        ok &= valid[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    cells[1:-1, 1:-1, 1:-1] = ok
    o, h = np.asarray(origin, np.float64), float(np.float32(voxel))
    t64 = tsdf.astype(np.float64)
    out = []
    for dx, dy, dz in DIRECTIONS:
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        held = np.zeros(tsdf[lo].shape, bool)
        for oz in ((1,) if dz else (0, 1)):
            for oy in ((1,) if dy else (0, 1)):
                for ox in ((1,) if dx else (0, 1)):
                    held |= cells[oz:oz + nz - dz, oy:oy + ny - dy, ox:ox + nx - dx]
        k, j, i = np.nonzero(valid[lo] & valid[hi] & (inside[lo] != inside[hi]) & held)
        ta, tb = t64[k, j, i], t64[k + dz, j + dy, i + dx]
        f = ta / (ta - tb)
        a = o + h * np.stack([i, j, k], 1)
        out.append(a + h * np.array([dx, dy, dz], np.float64) * f[:, None])
    return np.concatenate(out)


def topology(faces, nV):
    """dict(E undirected edges, boundary: edges in one face, nonmanifold: edges in more than two, repeated_directed: directed edges that
    appear more than once, unreferenced: vertices no face names, euler: V - E + F)."""
    faces = np.asarray(faces, np.int64)
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    directed = d[:, 0] * max(nV, 1) + d[:, 1]
    lo, hi = d.min(1), d.max(1)
    und = lo * max(nV, 1) + hi
    _, dn = np.unique(directed, return_counts=True)
    _, un = np.unique(und, return_counts=True)
    used = np.zeros(nV, bool)
    used[faces.reshape(-1)] = True
    return dict(E=len(un), boundary=int((un == 1).sum()), nonmanifold=int((un > 2).sum()), repeated_directed=int((dn > 1).sum()),
                unreferenced=int((~used).sum()), euler=nV - len(un) + len(faces))


def signed_volume(verts, faces):
    a, b, c = (verts[faces[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------------------------------------- the analytic grids
GRID = (17, 13, 11)                    # nx, ny, nz
CENTRE = (8.2, 6.1, 5.3)               # in node units
GRID_ORIGIN, GRID_VOXEL = (-0.7, 0.3, 1.1), 0.25


def _node_coords(dims=GRID):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i.astype(np.float64), j.astype(np.float64), k.astype(np.float64)


def _colors(dims=GRID):
    nx, ny, nz = dims
    return np.random.RandomState(5).rand(3, nz, ny, nx).astype(np.float32)


def sphere_grid(radius=3.7, cut_x=None):
    """(tsdf, weight, color) float32: distance to a sphere about CENTRE minus its radius, every node observed once — or, with cut_x, the
    node column x == cut_x never observed (weight 0, and a tsdf that must not be read)."""
    i, j, k = _node_coords()
    tsdf = (np.sqrt((i - CENTRE[0]) ** 2 + (j - CENTRE[1]) ** 2 + (k - CENTRE[2]) ** 2) - radius).astype(np.float32)
    weight = np.ones_like(tsdf)
    if cut_x is not None:
        weight[:, :, cut_x] = 0
        tsdf[:, :, cut_x] = -tsdf[:, :, cut_x]
    return tsdf, weight, _colors()


def torus_grid(R=4.3, r=1.6):
    i, j, k = _node_coords()
    q = np.sqrt((i - CENTRE[0]) ** 2 + (j - CENTRE[1]) ** 2) - R
    tsdf = (np.sqrt(q ** 2 + (k - CENTRE[2]) ** 2) - r).astype(np.float32)
    return tsdf, np.ones_like(tsdf), _colors()


# ------------------------------------------------------------------------------------------------- random lattices
U32 = 2.0 ** -24                       # float32's unit roundoff


def extract_bounds(ends, voxel):
    """(position bound [nV, 3], colour bound [nV, 3] | None) on |device - extract()| per component, from the kernel's arithmetic and not
    from its results: a = fma(voxel, i, o) and b likewise (one rounding each), f = ta / (ta - tb) (two; ta and tb differ in sign, so
    nothing cancels), a + (b - a) * f (a difference of at most one voxel, a product and a sum, or one fma): four roundings of a quantity
    no larger than max(|a|, |b|) and four of one no larger than the voxel; for colours four of one no larger than max(|ca|, |cb|)."""
    h = float(np.float32(voxel))
    pos = U32 * (4.0 * np.maximum(np.abs(ends.a), np.abs(ends.b)) + 4.0 * h)
    col = None if ends.ca is None else U32 * 4.0 * np.maximum(np.abs(ends.ca), np.abs(ends.cb))
    return pos, col


def random_lattice(dims, seed, p_invalid=0.0, specials=True):
    """(tsdf, weight, color) float32 of a grid with no structure at all.  tsdf: magnitudes uniform in [0.05, 1] with a random sign; with
    `specials` about 3 % of the nodes hold 0.0 and about 2 % hold -0.0 (both outside).  weight: a fraction p_invalid of the nodes draws
    from {0, 0.5, NaN} (invalid at min_weight = 1), the rest from {1, 2} (1 == min_weight is valid)."""
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    rs = np.random.RandomState(seed)
    tsdf = (rs.uniform(0.05, 1.0, shape) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)
    if specials:
        u = rs.rand(*shape)
        tsdf[u < 0.03] = np.float32(0.0)
        tsdf[(u >= 0.03) & (u < 0.05)] = np.float32(-0.0)
    invalid = rs.rand(*shape) < p_invalid
    weight = np.where(invalid, rs.choice([0.0, 0.5, np.nan], shape), rs.choice([1.0, 2.0], shape)).astype(np.float32)
    return tsdf, weight, rs.rand(3, *shape).astype(np.float32)


def with_outside_border(grid):
    """The grid with every border node outside (|tsdf|; a zero stays a zero): its surface cannot leave the grid, so it is closed."""
    tsdf, weight, color = grid
    tsdf = tsdf.copy()
    inner = np.zeros(tsdf.shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    tsdf[~inner] = np.abs(tsdf[~inner])
    return tsdf, weight, color


CONFIG_DIMS = (2, 2, 768)


def config_lattice():
    """(tsdf, weight, color) of a 2 x 2 x 768 grid that holds each of the 256 inside/outside configurations of a cell's corners once: cell
    c sits in slices 3c and 3c + 1, its corner (x, y, z) is inside iff bit x + 2y + 4z of c is set, the eight magnitudes of a cell differ;
    slice 3c + 2 is invalid (weight 0, NaN or 0.5 by turns) and holds tsdf values that must not be read."""
    nx, ny, nz = CONFIG_DIMS
    tsdf, weight = np.zeros((nz, ny, nx), np.float32), np.ones((nz, ny, nx), np.float32)
    for c in range(256):
        for z, y, x in itertools.product((0, 1), repeat=3):
            bit = x + 2 * y + 4 * z
            mag = (1 + (bit * 5 + c) % 8 + 8 * ((bit + c // 8) % 3)) / 32.0            # distinct within a cell: (bit * 5 + c) % 8 is a bijection
            tsdf[3 * c + z, y, x] = -mag if (c >> bit) & 1 else mag
        tsdf[3 * c + 2] = -tsdf[3 * c + 1] * 3
        weight[3 * c + 2] = (0.0, np.nan, 0.5)[c % 3]
    return tsdf, weight, np.random.RandomState(6).rand(3, nz, ny, nx).astype(np.float32)


def stacked(blocks, order, gap):
    """(tsdf, weight, color, k0): the lattices blocks[order[0]], blocks[order[1]], ... (each (tsdf, weight, color) with one nx and ny) one
    behind the other along z with `gap` >= 1 invalid slices (weight 0; tsdf -1, never read) between two of them; k0[n] is the first slice
    of the n-th.  No cell and no lattice edge with two valid ends crosses a gap, so the mesh is stacked_mesh()'s composition."""
    assert gap >= 1
    none = lambda like: (np.full((gap,) + like.shape[1:], -1, np.float32), np.zeros((gap,) + like.shape[1:], np.float32))
    ts, ws, cs, k0, at = [], [], [], [], 0
    for n, b in enumerate(order):
        tsdf, weight, color = blocks[b]
        if n:
            gt, gw = none(tsdf)
            ts.append(gt)
            ws.append(gw)
            cs.append(np.full((3,) + gt.shape, 0.5, np.float32))
            at += gap
        ts.append(tsdf)
        ws.append(weight)
        cs.append(color)
        k0.append(at)
        at += tsdf.shape[0]
    return np.concatenate(ts), np.concatenate(ws), np.concatenate(cs, 1), np.array(k0)


def stacked_mesh(blocks, order, k0, origin, voxel, min_weight=1.0):
    """(verts, colors, faces, ends) of stacked()'s grid, composed from one extract() per distinct block: faces concatenated with each
    block's vertex offset added, vertices (and the ends of their edges) shifted by float64(float32(voxel)) * k0 along z."""
    own = {b: extract(*blocks[b], origin, voxel, min_weight, ends=True) for b in sorted(set(order))}
    h = float(np.float32(voxel))
    V, C, F, A, B, CA, CB, nV = [], [], [], [], [], [], [], 0
    for b, k in zip(order, k0):
        v, c, f, e = own[b]
        shift = np.array([0.0, 0.0, h * float(k)])
        V.append(v + shift)
        A.append(e.a + shift)
        B.append(e.b + shift)
        C.append(c)
        CA.append(e.ca)
        CB.append(e.cb)
        F.append(f.astype(np.int64) + nV)
        nV += len(v)
    cat = np.concatenate
    return cat(V), cat(C), cat(F).astype(np.int32), Ends(cat(A), cat(B), cat(CA), cat(CB))


COLUMN_NX, COLUMN_NY, COLUMN_SLICES, COLUMN_GAP, COLUMN_UNITS = 6, 5, 12, 2, 716
COLUMN_ORIGIN, COLUMN_VOXEL = (0.3, -0.2, 0.1), 0.0004          # 10022 slices: a z extent of 4.0
SPINE_ROUND = 1024 * 256                                         # nodes (or faces, or vertices) behind which the scan's second round begins


def long_column(seed=7):
    """(blocks, order, gap) for stacked(): a 6 x 5 column of 716 random lattices of 12 slices with 2-slice gaps, 300 660 nodes in 1175
    blocks of 256, so that the one-block scan of the block sums runs a second round of 151 blocks.  Eight distinct lattices: five sparse
    (p_invalid = 0.2, 150 to 390 faces each) in a seeded order up to the one that holds node 262 144, three dense (every node valid,
    about 1640 faces each) in a seeded order from there on: the dense tail is what puts more than 40 % of all faces behind the first
    round, while the sparse front still passes 2^16 faces and vertices near block 400."""
    dims = (COLUMN_NX, COLUMN_NY, COLUMN_SLICES)
    blocks = [random_lattice(dims, 40 + n, p, True) for n, p in enumerate((0.2, 0.2, 0.2, 0.2, 0.2, 0.0, 0.0, 0.0))]
    straddles = SPINE_ROUND // (COLUMN_NX * COLUMN_NY) // (COLUMN_SLICES + COLUMN_GAP)
    rs = np.random.RandomState(seed)
    order = [int(rs.randint(0, 5)) if u < straddles else int(rs.randint(5, 8)) for u in range(COLUMN_UNITS)]
    return blocks, order, COLUMN_GAP


def _classes(tsdf, weight, min_weight):
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        valid = weight >= np.float32(min_weight)
        inside = tsdf < np.float32(0)
    ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        ok &= valid[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    return valid, inside, ok


def coverage(tsdf, weight, min_weight=1.0):
    """(pairs, configs) the valid cells of a grid reach: the set of (tetrahedron, inside mask over p0..p3), 96 at most, and the set of
    corner configurations (bit x + 2y + 4z), 256 at most.  Only there to assert that an input reaches what it is meant to."""
    valid, inside, ok = _classes(tsdf, weight, min_weight)
    nz, ny, nx = inside.shape
    corner = lambda x, y, z: inside[z:nz - 1 + z, y:ny - 1 + y, x:nx - 1 + x][ok].astype(np.int64)
    config = sum(corner(x, y, z) << (x + 2 * y + 4 * z) for z, y, x in itertools.product((0, 1), repeat=3))
    pairs = set()
    for t in range(6):
        mask = sum(corner(*p) << v for v, p in enumerate(tet_corners(t)))
        pairs |= {(t, int(m)) for m in np.unique(mask)}
    return pairs, {int(c) for c in np.unique(config)}


def held_classes(tsdf, weight, min_weight=1.0):
    """dict(none, some, all): the lattice edges whose two ends are valid and differ in `inside`, split by how many of the cells of the
    grid that contain the edge are valid.  Only `none` carries no vertex."""
    valid, inside, ok = _classes(tsdf, weight, min_weight)
    nz, ny, nx = inside.shape
    cells = np.zeros((nz + 1, ny + 1, nx + 1), np.int64)            # cell c at index c + 1, no cell beyond the borders
    exists = np.zeros_like(cells)
    cells[1:-1, 1:-1, 1:-1] = ok
    exists[1:-1, 1:-1, 1:-1] = 1
    out = dict(none=0, some=0, all=0)
    for dx, dy, dz in DIRECTIONS:
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        held, around = np.zeros(inside[lo].shape, np.int64), np.zeros(inside[lo].shape, np.int64)
        for oz, oy, ox in itertools.product(((1,) if dz else (0, 1)), ((1,) if dy else (0, 1)), ((1,) if dx else (0, 1))):
            at = (slice(oz, oz + nz - dz), slice(oy, oy + ny - dy), slice(ox, ox + nx - dx))
            held += cells[at]
            around += exists[at]
        cand = valid[lo] & valid[hi] & (inside[lo] != inside[hi])
        out["none"] += int((cand & (held == 0)).sum())
        out["all"] += int((cand & (held == around)).sum())
        out["some"] += int((cand & (held > 0) & (held < around)).sum())
    return out


# ------------------------------------------------------------------------------------------------- integration
class Volume:
    """The planes of a volume as float64 arrays (the device's are float32)."""

    def __init__(self, dims, origin, voxel, color=True, origin_exact=False):
        """origin_exact: keep `origin` in float64 (a crop of a larger volume, whose nodes lie at the larger volume's float32 origin plus
        whole voxels); otherwise it is rounded to float32 as the device's is."""
        nx, ny, nz = dims
        self.dims, self.voxel = dims, np.float32(voxel)
        self.origin = np.asarray(origin, np.float64) if origin_exact else np.asarray(origin, np.float32)
        self.tsdf, self.weight = np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx))
        self.color = np.zeros((3, nz, ny, nx)) if color else None


def integrate(vol, depth, rgb, alpha, alpha_min, viewmatrix, projmatrix, sdf_trunc, depth_trunc):
    """One view (include/gsr_hip_mesh.h, steps 1-5) in float64 on the float32 inputs.  Returns (written, unstable): the nodes the view
    updated, and the nodes at which a float32 evaluation may decide a skip rule differently (tests leave those out):
    px or py within 1e-3 of a half-integer, sdf within 1e-4 * sdf_trunc of -sdf_trunc, z, p.w or depth_trunc - d within 1e-5 of zero."""
    nx, ny, nz = vol.dims
    H, W = depth.shape
    o, h = vol.origin.astype(np.float64), float(vol.voxel)
    X, Y, Z = o[0] + h * np.arange(nx), o[1] + h * np.arange(ny), o[2] + h * np.arange(nz)
    V, P = np.asarray(viewmatrix, np.float32).astype(np.float64).reshape(-1), np.asarray(projmatrix, np.float32).astype(np.float64).reshape(-1)
    sdf_trunc, depth_trunc, alpha_min = float(np.float32(sdf_trunc)), float(np.float32(depth_trunc)), float(np.float32(alpha_min))
    depth64, alpha64 = depth.astype(np.float64).reshape(-1), None if alpha is None else alpha.astype(np.float64).reshape(-1)
    rgb64 = None if vol.color is None else [rgb[c].astype(np.float64).reshape(-1) for c in range(3)]
    written, unstable = np.zeros((nz, ny, nx), bool), np.zeros((nz, ny, nx), bool)
    near_tie = lambda q: np.abs(q - np.floor(q) - 0.5) < 1e-3
    slab = max(1, 65536 // (nx * ny))          # slices of z per round: arrays that stay in the cache (a 201^3 volume is walked in 201 rounds)
    for k0 in range(0, nz, slab):
        k1 = min(nz, k0 + slab)
        # each dot product is a sum of one term per axis: formed by broadcasting; what follows runs on the nodes still in play only
        dot = lambda cx, cy, cz, c0: (cx * X)[None, None, :] + (cy * Y)[None, :, None] + (cz * Z[k0:k1] + c0)[:, None, None]
        z, pw = dot(V[2], V[6], V[10], V[14]).reshape(-1), dot(P[3], P[7], P[11], P[15]).reshape(-1)
        flag = unstable[k0:k1].reshape(-1)        # (views of the slab: written through)
        flag |= (np.abs(z) < 1e-5) | (np.abs(pw) < 1e-5)
        at = np.nonzero((z > 0) & (pw > 0))[0]
        if len(at) == 0:
            continue
        z, pw = z[at], pw[at]
        px = ((dot(P[0], P[4], P[8], P[12]).reshape(-1)[at] / pw + 1.0) * W - 1.0) / 2.0
        py = ((dot(P[1], P[5], P[9], P[13]).reshape(-1)[at] / pw + 1.0) * H - 1.0) / 2.0
        flag[at[(near_tie(px) | near_tie(py)) & (px > -2) & (px < W + 1) & (py > -2) & (py < H + 1)]] = True
        u, v = np.rint(px), np.rint(py)
        keep = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        at, z, pix = at[keep], z[keep], (v[keep] * W + u[keep]).astype(np.int64)
        d = depth64[pix]
        flag[at[np.abs(depth_trunc - d) < 1e-5]] = True
        with np.errstate(invalid="ignore"):
            keep = (d > 0) & (d <= depth_trunc)
            if alpha64 is not None:
                keep &= alpha64[pix] >= alpha_min
        at, z, pix, d = at[keep], z[keep], pix[keep], d[keep]
        sdf = d - z
        flag[at[np.abs(sdf + sdf_trunc) < 1e-4 * sdf_trunc]] = True
        keep = ~(sdf < -sdf_trunc)
        at, pix, sdf = at[keep], pix[keep], sdf[keep]
        t = np.minimum(1.0, sdf / sdf_trunc)
        tsdf, weight = vol.tsdf[k0:k1].reshape(-1), vol.weight[k0:k1].reshape(-1)
        w = weight[at]
        tsdf[at] = (tsdf[at] * w + t) / (w + 1.0)
        if vol.color is not None:
            for c in range(3):
                plane = vol.color[c, k0:k1].reshape(-1)
                plane[at] = (plane[at] * w + rgb64[c][pix]) / (w + 1.0)
        weight[at] = w + 1.0
        written[k0:k1].reshape(-1)[at] = True
    return written, unstable


def ray_depth_map(cam, centre, radius, plane_n, plane_h):
    """The view-space depth each pixel centre of `cam` (a camera dictionary of tests/cameras.py) sees of a sphere in front of the plane
    {X: n . X = h}, 0 where the ray meets neither.  Pixel (u, v) looks along ((u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy, 1)."""
    W, H, K = cam["W"], cam["H"], cam["K"].astype(np.float64)
    R, T = cam["R"].astype(np.float64), cam["T"].astype(np.float64)           # view = R^T X + T
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(u + 0.5 - K[0, 2]) / K[0, 0], (v + 0.5 - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
    c = R.T @ np.asarray(centre, np.float64) + T
    n = R.T @ np.asarray(plane_n, np.float64)
    hv = plane_h + n @ T                                                        # n . X = h  <=>  n_view . p_view = h + n_view . T
    with np.errstate(all="ignore"):
        t_plane = hv / (ray @ n)
        t_plane = np.where(t_plane > 0, t_plane, np.inf)
        A, B, C = (ray * ray).sum(-1), ray @ c, c @ c - radius * radius
        disc = B * B - A * C
        t_sphere = np.where(disc > 0, (B - np.sqrt(np.maximum(disc, 0))) / A, np.inf)
        t_sphere = np.where(t_sphere > 0, t_sphere, np.inf)
    t = np.minimum(t_plane, t_sphere)
    return np.where(np.isfinite(t), t, 0.0).astype(np.float32)


FIX_DIMS, FIX_VOXEL, FIX_ORIGIN = (23, 19, 17), 0.1, (-1.3, -0.8, -0.25)
FIX_W, FIX_H = 61, 45
FIX_SDF_TRUNC, FIX_DEPTH_TRUNC, FIX_ALPHA_MIN = 0.25, 1.3, 0.5
FIX_VIEWS = (("offcentre", 20), ("rolled", 30), ("aniso", 10))


def integrate_fixture():
    """[dict(cam, depth, rgb, alpha)] of the three views: a sphere in front of a slanted plane inside the box of FIX_*, rows 10-12 of each
    depth map zero, one NaN pixel, alpha 0.3 over the top-left corner, random rgb."""
    import cameras
    views = []
    for n, (name, seed) in enumerate(FIX_VIEWS):
        cam = cameras.family(name, FIX_W, FIX_H, seed)
        depth = ray_depth_map(cam, (-0.2, 0.1, 0.8), 0.3, np.array([0.3, 0.0, 1.0]) / math.hypot(0.3, 1.0), 1.1)
        depth[10:13] = 0.0
        depth[20, 30] = np.nan
        alpha = np.ones((FIX_H, FIX_W), np.float32)
        alpha[:12, :15] = 0.3
        rgb = np.random.RandomState(40 + n).rand(3, FIX_H, FIX_W).astype(np.float32)
        views.append(dict(cam=cam, depth=depth, rgb=rgb, alpha=alpha))
    return views


def integrate_reference(views=None, color=True):
    """[(tsdf, weight, color, written, unstable so far)] after one, two and three views of the fixture (copies)."""
    views = integrate_fixture() if views is None else views
    vol = Volume(FIX_DIMS, FIX_ORIGIN, FIX_VOXEL, color)
    unstable = np.zeros(vol.tsdf.shape, bool)
    out = []
    for vw in views:
        written, uns = integrate(vol, vw["depth"], vw["rgb"] if color else None, vw["alpha"], FIX_ALPHA_MIN, vw["cam"]["viewmatrix"],
                                 vw["cam"]["projmatrix"], FIX_SDF_TRUNC, FIX_DEPTH_TRUNC)
        unstable = unstable | uns
        out.append((vol.tsdf.copy(), vol.weight.copy(), None if vol.color is None else vol.color.copy(), written, unstable.copy()))
    return out


# ------------------------------------------------------------------------------------------------- PLY
def read_ply(path):
    """A reader of its own for what gsr_mesh.save_mesh_ply writes: (verts f32 [nV,3], colors u8 [nV,3] | None, faces i32 [nT,3])."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nV = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[-1])
    nT = int(next(ln for ln in lines if ln.startswith("element face")).split()[-1])
    has_color = "property uchar red" in lines
    vt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if has_color else []))
    ft = np.dtype([("n", "u1"), ("i", "<i4", 3)])
    v = np.frombuffer(body, vt, nV)
    f = np.frombuffer(body, ft, nT, offset=nV * vt.itemsize)
    assert len(body) == nV * vt.itemsize + nT * ft.itemsize and (f["n"] == 3).all()
    return v["p"].copy(), (v["c"].copy() if has_color else None), f["i"].copy()
