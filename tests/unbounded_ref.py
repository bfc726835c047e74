"""float64 numpy restatement of include/gsr_hip_unbounded.h (test infrastructure only): the contraction and its inverse, TSDF integration
of one view into a lattice in contracted space, per-point colouring from one view, and the un-contraction of points.  Inputs are the
float32-rounded arrays and scalars the device gets; every decision (the skip rules, the taps, the clamps) follows the header, the
arithmetic is float64.  The iso-surface is mesh_ref.extract's.

  contract_norm / contract / uncontract / trunc_of      the contraction on norms and points, the truncation of a node at norm m
  Lattice(n, extent, centre, radius)                    the planes of a ContractedTSDFVolume as float64 arrays, fresh: tsdf = weight = 1
  observe(X, depth, V, P, trunc)                        steps 2-4 for world points: (ok, t, taps, unstable)
  integrate(lat, depth, viewmatrix, projmatrix)      -> (written [n,n,n] bool, unstable [n,n,n] bool); lat's planes are updated in place
  fuse_points(points, color, weight, depth, rgb, ...) -> (written [m] bool, unstable [m] bool); color and weight are updated in place
  uncontract_points(src, centre, radius, max_range)  -> [m, 3] float64
  fixture_reference(n, extent)                          [(tsdf, weight, written, unstable so far)] after one, two and three fixture views
  axis_cameras / ball_scene                             six cameras on the axes about a centre; the analytic scene of the end-to-end tests

`unstable` marks the elements at which a float32 evaluation may decide a skip rule differently (tests leave those out): | m - 2 | < 1e-4,
| z | or | p.w | < 1e-5, | q.x | or | q.y | within 1e-5 of 1, sdf within 1e-4 * trunc of -trunc.  Nothing else in the contract is a
threshold on computed values: the clamps and the floor are continuous in the result, and the taps are compared as data.
"""
import math

import numpy as np

import mesh_ref as M

BELOW_TWO = float(np.nextafter(np.float32(2), np.float32(0)))


# ------------------------------------------------------------------------------------------------- the contraction
def contract_norm(m):
    """The contracted norm of a point at norm m: m inside the unit ball, 2 - 1 / m beyond."""
    m = np.asarray(m, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(m <= 1, m, 2 - 1 / m)


def contract(x):
    x = np.asarray(x, np.float64)
    m = np.linalg.norm(x, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(m <= 1, x, x * (2 - 1 / m) / m)


def uncontract_scale(m):
    """x = y * uncontract_scale(|y|) for |y| < 2."""
    m = np.asarray(m, np.float64)
    with np.errstate(all="ignore"):
        return np.where(m <= 1, 1.0, 1 / (m * (2 - m)))


def uncontract(y):
    y = np.asarray(y, np.float64)
    return y * uncontract_scale(np.linalg.norm(y, axis=-1, keepdims=True))


def trunc_of(m, voxel):
    m = np.asarray(m, np.float64)
    return np.where(m <= 1, 5 * voxel, 5 * voxel / (2 - np.minimum(m, 1.9)))


# ------------------------------------------------------------------------------------------------- integration
class Lattice:
    """The lattice gsr_mesh.ContractedTSDFVolume(centre, radius, n, extent) lays out, its scalars rounded to float32 as the device gets
    them, its planes float64 and fresh (tsdf = weight = 1)."""

    def __init__(self, n, extent, centre, radius):
        self.n = int(n)
        f32 = lambda v: float(np.float32(v))
        self.lo, self.step, self.voxel = f32(-extent), f32(2.0 * extent / (n - 1)), f32(2.0 * radius / n)
        self.centre, self.radius = np.asarray(centre, np.float32).astype(np.float64), f32(radius)
        self.tsdf, self.weight = np.ones((n, n, n)), np.ones((n, n, n))

    def axis(self):
        """The contracted coordinate of node i along one axis: fmaf(step, i, lo) rounded to float32."""
        return (self.step * np.arange(self.n) + self.lo).astype(np.float32).astype(np.float64)

    def nodes(self):
        """y [n, n, n, 3] (z, y, x index order; components x, y, z)."""
        a = self.axis()
        k, j, i = np.meshgrid(a, a, a, indexing="ij")
        return np.stack([i, j, k], -1)


def observe(X, depth, viewmatrix, projmatrix, trunc):
    """Steps 2-4 of the header for world points X [m, 3] with truncation trunc [m] (or a scalar): (ok [m] bool, t [m], taps, unstable
    [m] bool); taps = (i00, i01, i10, i11 flat pixel indices, a, b), to sample further planes with.  t is meaningful where ok."""
    H, W = depth.shape
    V, P = np.asarray(viewmatrix, np.float32).astype(np.float64).reshape(-1), np.asarray(projmatrix, np.float32).astype(np.float64).reshape(-1)
    trunc = np.broadcast_to(np.asarray(trunc, np.float64), X.shape[:1])
    dot = lambda A, r: X[:, 0] * A[r] + X[:, 1] * A[4 + r] + X[:, 2] * A[8 + r] + A[12 + r]
    z, pw = dot(V, 2), dot(P, 3)
    unstable = (np.abs(z) < 1e-5) | (np.abs(pw) < 1e-5)
    ok = (z > 0) & (pw > 0)
    with np.errstate(all="ignore"):
        qx, qy = dot(P, 0) / pw, dot(P, 1) / pw
        unstable |= ok & ((np.abs(np.abs(qx) - 1) < 1e-5) | (np.abs(np.abs(qy) - 1) < 1e-5))
        ok &= (qx > -1) & (qx < 1) & (qy > -1) & (qy < 1)
        px = np.clip(np.where(ok, ((qx + 1) * W - 1) / 2, 0.0), 0, W - 1)
        py = np.clip(np.where(ok, ((qy + 1) * H - 1) / 2, 0.0), 0, H - 1)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    a, b = px - x0, py - y0
    taps = (y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1, a, b)
    d64 = depth.astype(np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        for at in taps[:4]:
            ok &= d64[at] > 0                      # (a NaN tap: False)
        d = sample(d64, taps)
        sdf = d - z
        unstable |= ok & (np.abs(sdf + trunc) < 1e-4 * trunc)
        ok &= sdf > -trunc
        t = np.clip(sdf / trunc, -1, 1)
    return ok, t, taps, unstable


def sample(plane, taps):
    """The bilinear blend of a flat float64 plane at observe()'s taps."""
    i00, i01, i10, i11, a, b = taps
    return (plane[i00] * (1 - a) + plane[i01] * a) * (1 - b) + (plane[i10] * (1 - a) + plane[i11] * a) * b


def integrate(lat, depth, viewmatrix, projmatrix):
    """One view into the lattice (gsr_tsdf_integrate_contracted, steps 1-5)."""
    n = lat.n
    y = lat.nodes().reshape(-1, 3)
    m = np.linalg.norm(y, axis=1)
    unstable = np.abs(m - 2) < 1e-4
    live = m < 2
    X = lat.centre + lat.radius * (y * uncontract_scale(np.where(live, m, 1.0))[:, None])
    ok, t, _, uns = observe(X, depth, viewmatrix, projmatrix, trunc_of(m, lat.voxel))
    unstable |= live & uns
    ok &= live
    tsdf, weight = lat.tsdf.reshape(-1), lat.weight.reshape(-1)
    w = weight[ok]
    tsdf[ok] = (tsdf[ok] * w + t[ok]) / (w + 1)
    weight[ok] = w + 1
    return ok.reshape(n, n, n), unstable.reshape(n, n, n)


def fuse_points(points, color, weight, depth, rgb, viewmatrix, projmatrix, sdf_trunc):
    """One view into per-point colours (gsr_points_fuse_view): points [m, 3] float32, color [m, 3] and weight [m] float64, in place."""
    X = np.asarray(points, np.float32).astype(np.float64)
    ok, _, taps, unstable = observe(X, depth, viewmatrix, projmatrix, float(np.float32(sdf_trunc)))
    w = weight[ok]
    kept = tuple(t[ok] for t in taps)
    for c in range(3):
        color[ok, c] = (color[ok, c] * w + sample(rgb[c].astype(np.float64).reshape(-1), kept)) / (w + 1)
    weight[ok] = w + 1
    return ok, unstable


def uncontract_points(src, centre, radius, max_range):
    """gsr_uncontract_points: a point with m >= 2 takes the largest float32 below 2 in the divisor."""
    y = np.asarray(src, np.float32).astype(np.float64)
    m = np.linalg.norm(y, axis=1)
    with np.errstate(invalid="ignore"):
        m = np.where(m < 2, m, BELOW_TWO)
    c, r, R = np.asarray(centre, np.float32).astype(np.float64), float(np.float32(radius)), float(np.float32(max_range))
    return np.clip(c + r * (y * uncontract_scale(m)[:, None]), -R, R)


# ------------------------------------------------------------------------------------------------- the fixture
FIX_CENTRE, FIX_RADIUS = (-0.2, 0.1, 0.8), 0.5          # the sphere of mesh_ref.integrate_fixture() sits at the centre
FIX_LATTICES = ((33, 1.9), (24, 1.5))                   # (n, extent)


def fixture_reference(n, extent, views=None):
    """[(tsdf, weight, written, unstable so far)] after one, two and three views of mesh_ref.integrate_fixture() (copies)."""
    views = M.integrate_fixture() if views is None else views
    lat = Lattice(n, extent, FIX_CENTRE, FIX_RADIUS)
    unstable = np.zeros((n, n, n), bool)
    out = []
    for vw in views:
        written, uns = integrate(lat, vw["depth"], vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"])
        unstable = unstable | uns
        out.append((lat.tsdf.copy(), lat.weight.copy(), written, unstable.copy()))
    return out


def fixture_points(count=5000, seed=9):
    """Seeded world points [count, 3] float32 around the fixture's sphere (half of them, within 0.1 of its surface) and its slanted
    plane (the rest, within 0.1 of it)."""
    rs = np.random.RandomState(seed)
    half = count // 2
    d = rs.randn(half, 3)
    on_sphere = np.asarray(FIX_CENTRE) + d / np.linalg.norm(d, axis=1, keepdims=True) * (0.3 + rs.uniform(-0.1, 0.1, (half, 1)))
    nrm = np.array([0.3, 0.0, 1.0]) / math.hypot(0.3, 1.0)
    xy = rs.uniform(-1.2, 1.0, (count - half, 2))
    on_plane = np.stack([xy[:, 0], xy[:, 1], (1.1 - nrm[0] * xy[:, 0]) / nrm[2]], 1) + nrm * rs.uniform(-0.1, 0.1, (count - half, 1))
    return np.concatenate([on_sphere, on_plane]).astype(np.float32)


# ------------------------------------------------------------------------------------------------- analytic scenes
def axis_cameras(W, H, centre, distance, fov_deg=70.0):
    """Six camera dictionaries (tests/cameras.py) at centre +- distance * e_x, e_y, e_z, each looking at the centre."""
    import cameras
    centre = np.asarray(centre, np.float64)
    f = W / (2.0 * math.tan(math.radians(fov_deg) / 2.0))
    out = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = np.zeros(3)
            d[axis] = sign
            fwd = -d
            up = np.eye(3)[(axis + 1) % 3]
            right = np.cross(up, fwd)
            down = np.cross(fwd, right)
            R = np.stack([right, down, fwd], 1)                      # camera-to-world: the columns are the camera's axes
            out.append(cameras.hwk_camera(W, H, f, f, W / 2.0, H / 2.0, R=R, T=-R.T @ (centre + distance * d)))
    return out


BALL_CENTRE, BALL_RADIUS, BALL_RHO, BALL_FLOOR = (0.1, -0.2, 0.3), 1.0, 0.5, -1.5


def ball_scene(W=96, H=96):
    """[(cam, depth)] of the end-to-end scene: six cameras on the unit sphere about BALL_CENTRE (so camera_bounds() would give that
    sphere) see a ball of radius BALL_RHO at the centre, inside the unit ball, in front of the floor z = centre.z + BALL_FLOOR, which
    lies in the shell and runs on without end.  Every camera is above the floor."""
    cams = axis_cameras(W, H, BALL_CENTRE, BALL_RADIUS, fov_deg=90.0)
    n, h = np.array([0.0, 0.0, 1.0]), BALL_CENTRE[2] + BALL_FLOOR
    out = []
    for cam in cams:
        depth = M.ray_depth_map(cam, BALL_CENTRE, BALL_RHO, n, h)
        depth[depth > 50] = 0                                        # rays that run along the floor
        out.append((cam, depth))
    return out


def ball_distance(X):
    """Distance of world points to the end-to-end scene's surface: the ball or the floor, whichever is nearer."""
    X = np.asarray(X, np.float64) - np.asarray(BALL_CENTRE)
    return np.minimum(np.abs(np.linalg.norm(X, axis=1) - BALL_RHO), np.abs(X[:, 2] - BALL_FLOOR))
