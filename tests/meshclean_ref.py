"""Integer restatement of include/gsr_hip_meshclean.h in numpy (test infrastructure only), and the fixtures of the clean-up tests.

  clean(verts, faces, colors, cluster_to_keep, min_triangles[, labels]) -> Cleaned(verts, faces, colors, tri_label, tri_size, counts)
        counts = (nV_out, nT_out, C, kept components, thr, ignored faces), the six the device writes
  labels_by_scipy(faces, nV)    the labels once more from scipy.sparse.csgraph.connected_components, where scipy is installed
  two_spheres() / chain() / singles() / scrambled()      the fixtures: (verts f32 [nV,3], faces i32 [nT,3], colors f32 [nV,3])
  strips() / star() / sheet() / interleaved() / with_duplicates()      chains of given sizes, faces about one hub, a triangulated grid,
                                two chains on the even and odd indices, repeated faces

Everything is exact: labels, sizes and counts are integers, and the rows of vertices and colours are gathered, not computed.
"""
import collections

import numpy as np

import mesh_ref as M

Cleaned = collections.namedtuple("Cleaned", "verts faces colors tri_label tri_size counts")


def counted_faces(faces, nV):
    """bool [nT]: the three indices lie in [0, nV) and are pairwise distinct."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < nV)).all(1)
    return ok & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def vertex_labels(faces, nV):
    """int64 [nV]: per vertex the smallest vertex index of its component, by a union-find of its own (the smaller root becomes the parent,
    so a root is the smallest index of its tree)."""
    parent = list(range(nV))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    for a, b, c in f[counted_faces(f, nV)].tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(nV)], np.int64)


def labels_by_scipy(faces, nV):
    """vertex_labels() from scipy's connected components (None without scipy): its arbitrary component numbers mapped to minima."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[counted_faces(f, nV)]
    rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    _, comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nV, nV)), directed=False)
    smallest = np.full(comp.max() + 1 if nV else 0, nV, np.int64)
    np.minimum.at(smallest, comp, np.arange(nV))
    return smallest[comp]


def clean(verts, faces, colors, cluster_to_keep, min_triangles, labels=None):
    """labels: vertex_labels(faces, nV) where the caller has them already (they do not depend on the two parameters)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nV, nT = len(verts), len(faces)
    assert cluster_to_keep >= 1 and min_triangles >= 0
    if nV == 0 or nT == 0:             # no component, no threshold; every face is ignored
        none = np.zeros((0, 3), np.float32)
        return Cleaned(none, np.zeros((0, 3), np.int32), None if colors is None else none.copy(), np.full(nT, -1, np.int32), np.zeros(nT, np.int32),
                       (0, 0, 0, 0, 0, nT))
    ok = counted_faces(faces, nV)
    label = vertex_labels(faces, nV) if labels is None else labels
    tri_label = np.where(ok, label[np.where(ok, faces[:, 0], 0)], -1)
    comp_size = np.bincount(tri_label[ok], minlength=nV)           # by label; zero where the vertex is no root or in no counted face
    tri_size = np.where(ok, comp_size[np.where(ok, tri_label, 0)], 0)
    sizes = np.sort(comp_size[comp_size >= 1])[::-1]               # s_1 >= s_2 >= ... >= s_C
    C = len(sizes)
    thr = max(int(sizes[min(cluster_to_keep, C) - 1]), min_triangles) if C else min_triangles
    keep = ok & (tri_size >= thr)
    used = np.zeros(nV, bool)
    used[faces[keep].reshape(-1)] = True
    new_row = np.cumsum(used) - 1
    counts = (int(used.sum()), int(keep.sum()), C, int((sizes >= thr).sum()), int(thr), int((~ok).sum()))
    return Cleaned(verts[used], new_row[faces[keep]].astype(np.int32), None if colors is None else np.asarray(colors, np.float32)[used],
                   tri_label.astype(np.int32), tri_size.astype(np.int32), counts)


# ------------------------------------------------------------------------------------------------- fixtures
FLOATERS = 10


def _sphere_mesh(radius):
    tsdf, weight, color = M.sphere_grid(radius)
    V, C, F = M.extract(tsdf, weight, color, M.GRID_ORIGIN, M.GRID_VOXEL)
    return V.astype(np.float32), F, C.astype(np.float32)


_two_spheres = []


def two_spheres():
    """(verts, faces, colors, parts): the sphere of mesh_ref.sphere_grid at radius 3.7 (the LARGER: vertices and faces first), a copy at
    radius 3.1 ten units along x, FLOATERS isolated triangles, and five vertices no face names (two in front, three at the end).
    parts = dict(big=(nV, nT), small=(nV, nT)).  Built once."""
    if not _two_spheres:
        (Va, Fa, Ca), (Vb, Fb, Cb) = _sphere_mesh(3.7), _sphere_mesh(3.1)
        assert len(Fa) > len(Fb) > 1000
        rs = np.random.RandomState(11)
        Vf = (rs.rand(3 * FLOATERS, 3) * 0.1 + np.repeat(np.arange(FLOATERS), 3)[:, None]).astype(np.float32)
        loose = rs.rand(5, 3).astype(np.float32)
        verts = np.concatenate([loose[:2], Va, Vb + np.float32([10, 0, 0]), Vf, loose[2:]])
        o = 2
        faces = np.concatenate([Fa + o, Fb + o + len(Va), np.arange(3 * FLOATERS, dtype=np.int32).reshape(-1, 3) + o + len(Va) + len(Vb)]).astype(np.int32)
        colors = np.concatenate([loose[:2], Ca, Cb, rs.rand(3 * FLOATERS, 3).astype(np.float32), loose[2:]])
        _two_spheres.append((verts, faces, colors, dict(big=(len(Va), len(Fa)), small=(len(Vb), len(Fb)))))
    return _two_spheres[0]


def scrambled(verts, faces, colors, seed):
    """The same mesh with its faces in a seeded random order and its vertex rows in a seeded random permutation."""
    rs = np.random.RandomState(seed)
    new_of_old = rs.permutation(len(verts))
    v, c = np.empty_like(verts), None if colors is None else np.empty_like(colors)
    v[new_of_old] = verts
    if colors is not None:
        c[new_of_old] = colors
    f = new_of_old[faces].astype(np.int32)[rs.permutation(len(faces))]
    return v, f, c


def chain(N, order, seed=5):
    """Vertices 0..N+1 and the N faces (i, i+1, i+2): one component; order = "ascending", "descending" or "shuffled"."""
    i = np.arange(N, dtype=np.int32)
    faces = np.stack([i, i + 1, i + 2], 1)
    if order == "descending":
        faces = faces[::-1]
    elif order == "shuffled":
        faces = faces[np.random.RandomState(seed).permutation(N)]
    else:
        assert order == "ascending"
    rs = np.random.RandomState(seed + 1)
    return rs.rand(N + 2, 3).astype(np.float32), np.ascontiguousarray(faces), rs.rand(N + 2, 3).astype(np.float32)


def _rows(nV, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(nV, 3).astype(np.float32), rs.rand(nV, 3).astype(np.float32)


def strips(sizes, seed=13):
    """Disjoint chains, one per entry of `sizes`: the n-th has sizes[n] faces (i, i+1, i+2) over sizes[n] + 2 vertices of its own, in
    the order given: component n has exactly sizes[n] faces."""
    faces, at = [], 0
    for n in sizes:
        i = np.arange(n, dtype=np.int64) + at
        faces.append(np.stack([i, i + 1, i + 2], 1))
        at += n + 2
    verts, colors = _rows(at, seed)
    return verts, np.concatenate(faces).astype(np.int32), colors


def star(n, hub, seed=14):
    """n faces (hub, a_i, b_i) over 2 n + 1 vertices that share the hub and nothing else: no two faces share an edge, all are one
    component.  hub = "first": the hub is vertex 0 (the root every union arrives at); "last": vertex 2 n (the one every union hangs)."""
    assert hub in ("first", "last")
    i = np.arange(n, dtype=np.int64)
    if hub == "first":
        faces = np.stack([np.zeros(n, np.int64), 1 + 2 * i, 2 + 2 * i], 1)
    else:
        faces = np.stack([np.full(n, 2 * n, np.int64), 2 * i, 2 * i + 1], 1)
    verts, colors = _rows(2 * n + 1, seed)
    return verts, faces.astype(np.int32), colors


def sheet(n, m, seed=15):
    """A grid of n x m quads, each cut into two triangles: (n + 1)(m + 1) vertices, 2 n m faces, one component."""
    j, i = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(m, dtype=np.int64), indexing="ij")
    v = (j * (m + 1) + i).reshape(-1)
    faces = np.stack([np.stack([v, v + 1, v + m + 2], 1), np.stack([v, v + m + 2, v + m + 1], 1)], 1).reshape(-1, 3)
    verts, colors = _rows((n + 1) * (m + 1), seed)
    return verts, faces.astype(np.int32), colors


def interleaved(n, drop=0, seed=16):
    """Two chains of n faces each, one over the even vertex indices (2i, 2i+2, 2i+4) and one over the odd (2i+1, 2i+3, 2i+5), their
    faces by turns: neighbouring indices lie in different components throughout.  drop: faces left off the END of the odd chain (its
    last vertices are then in no face)."""
    i = np.arange(n, dtype=np.int64)
    faces = np.stack([np.stack([2 * i, 2 * i + 2, 2 * i + 4], 1), np.stack([2 * i + 1, 2 * i + 3, 2 * i + 5], 1)], 1).reshape(-1, 3)
    keep = np.ones(2 * n, bool)
    if drop:
        keep[2 * (n - drop) + 1::2] = False
    verts, colors = _rows(2 * n + 4, seed)
    return verts, faces[keep].astype(np.int32), colors


def with_duplicates(verts, faces, colors, every=3, seed=17):
    """The mesh with every `every`-th face said once more, as the same triple or rotated, spliced in at seeded places: a repeat is a
    counted face like any other (a component's size counts it)."""
    rs = np.random.RandomState(seed)
    again = faces[::every].copy()
    turn = rs.randint(0, 3, len(again))
    again = again[np.arange(len(again))[:, None], (np.arange(3)[None, :] + turn[:, None]) % 3]
    at = np.sort(rs.randint(0, len(faces) + 1, len(again)))
    return verts, np.insert(faces, at, again, axis=0).astype(np.int32), colors


def singles(n=70000, fan=60, seed=9):
    """n single-triangle components, then one fan of `fan` faces about a hub (fan + 2 vertices)."""
    tri = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    hub = 3 * n
    k = np.arange(fan, dtype=np.int32)
    fan_faces = np.stack([np.full(fan, hub, np.int32), hub + 1 + k, hub + 2 + k], 1)
    rs = np.random.RandomState(seed)
    nV = 3 * n + fan + 2
    return rs.rand(nV, 3).astype(np.float32), np.concatenate([tri, fan_faces]), rs.rand(nV, 3).astype(np.float32)
