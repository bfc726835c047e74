"""The env-scope pass (include/gsr_hip_scope.h: gsr_env_scope_forward / _backward) and RawTrainState.dist_color restated in float64 numpy,
the band of squared distances in which a float32 evaluation may legitimately fall on either side of the sphere, and the point sets the
GPU tests use.  Not a test; tests/test_env_scope_ref.py pins it against the torch expressions it restates (float32 torch on the CPU) and
checks that the generators keep their promises.

The expressions (the reference's train.py, env-scope branch, and GaussianModel.dist_color):
    outside = sum((xyz - centre)^2, -1) > radius^2        inside = ... < radius^2 (render's env_scope_mask)
    loss    = refl[outside].mean()                         d loss / d refl[i] = 1 / count on outside rows, 0 elsewhere
    f_dc   += noise * noise_range * 2 - noise_range        on the rows outside exclusive_msk; moments of the whole f_dc group zeroed
"""
import numpy as np

U = 2.0 ** -24           # unit roundoff of float32
BAND = 8 * U             # relative half-width of the ambiguous band around radius2 (see band())

CLEAR_CENTRE, CLEAR_RADIUS = (0.3, -1.2, 2.5), 1.7
LATTICE_CENTRE, LATTICE_RADIUS = (1.0, 2.0, 3.0), 3.0


def centre32(centre):
    """The centre as the library receives it: rounded to float32 once (what torch.tensor(centre) holds), as float64."""
    return np.asarray([float(c) for c in centre], dtype=np.float32).astype(np.float64)


def radius2(radius):
    """The value both torch and the library compare against: the Python float radius ** 2 rounded to float32, as float64."""
    return np.float64(np.float32(float(radius) ** 2))


def d2(xyz, centre):
    """Squared distances in float64 from the float32 coordinates and the float32 centre."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((x - centre32(centre)[None]) ** 2).sum(axis=-1)


def band(xyz, centre, radius):
    """True where a correct float32 evaluation of d2 may land on either side of radius2 (or on it).  Every term of the float32 sum carries
    the subtraction's rounding twice (it is squared), the square's once and at most two additions': a factor within (1 + 2^-24)^5, a
    relative error of at most gamma_5 < 6 * 2^-24 of d2 — taken as |d2 - radius2| <= 8 * 2^-24 * max(d2, radius2), with margin.  Rows with
    a NaN or infinite d2 are never ambiguous."""
    q, r2 = d2(xyz, centre), radius2(radius)
    with np.errstate(invalid="ignore"):
        return np.isfinite(q) & (np.abs(q - r2) <= BAND * np.maximum(q, r2))


def masks(xyz, centre, radius):
    """(inside, outside) by the two plain comparisons in float64: d2 == radius2 and NaN are in neither, +-inf is outside."""
    q, r2 = d2(xyz, centre), radius2(radius)
    with np.errstate(invalid="ignore"):
        return q < r2, q > r2


def loss(refl, outside):
    """(sum, count, mean) over the outside rows in float64; the mean of an empty selection is NaN, as torch's."""
    r = np.asarray(refl, dtype=np.float32).astype(np.float64).reshape(-1)
    s, n = float(r[outside].sum()), int(outside.sum())
    return s, n, (s / n if n else float("nan"))


def gradient(outside, g=1.0):
    """d(g * mean)/d refl: g / count on outside rows, exactly 0 elsewhere; all zero for an empty selection (torch sends no gradient there)."""
    n = int(outside.sum())
    out = np.zeros(outside.shape[0], dtype=np.float64)
    if n:
        out[outside] = float(g) / n
    return out


def dist_color(f_dc, noise, noise_range=0.4, exclusive_msk=None):
    """New DC colours [P,3] in float64 from float32 inputs: f_dc + (noise * noise_range * 2 - noise_range), excluded rows as they were."""
    dc = np.asarray(f_dc, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    nz = np.asarray(noise, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    new = dc + (nz * noise_range * 2 - noise_range)
    if exclusive_msk is not None:
        new[exclusive_msk] = dc[exclusive_msk]
    return new


# ------------------------------------------------------------------------------------------------- point sets
def _directions(rs, n):
    v = rs.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def clear_points(P, seed=0):
    """(xyz float32 [P,3], refl float32 [P], centre, radius): distances from [0, 0.98 r] (even rows) and [1.02 r, 3 r] (odd rows), uniform
    directions about a centre off the origin.  The 2 % gap is 4 orders of magnitude wider than the band: no row is ambiguous, so every
    correct evaluation gives the same masks, and both masks hold about half of the rows."""
    rs = np.random.RandomState(seed)
    r = CLEAR_RADIUS
    u = rs.rand(P)
    dist = np.where(np.arange(P) % 2 == 0, 0.98 * r * u, 1.02 * r + (3.0 - 1.02) * r * u)
    xyz = (np.asarray(CLEAR_CENTRE)[None] + dist[:, None] * _directions(rs, P)).astype(np.float32)
    refl = rs.uniform(0.001, 0.999, P).astype(np.float32)
    return xyz, refl, CLEAR_CENTRE, CLEAR_RADIUS


def shell_points(P, seed=0):
    """(xyz, refl, centre, radius, side): points at r * (1 - 2^-18) (side -1, even rows) and r * (1 + 2^-18) (side +1, odd rows): 16 times
    closer to the sphere than anything in clear_points and still 16 band widths away from it."""
    rs = np.random.RandomState(seed + 1)
    side = np.where(np.arange(P) % 2 == 0, -1, 1)
    dist = CLEAR_RADIUS * (1.0 + side * 2.0 ** -18)
    xyz = (np.asarray(CLEAR_CENTRE)[None] + dist[:, None] * _directions(rs, P)).astype(np.float32)
    refl = rs.uniform(0.001, 0.999, P).astype(np.float32)
    return xyz, refl, CLEAR_CENTRE, CLEAR_RADIUS, side


# offsets from LATTICE_CENTRE whose squares are small integers: d2 is exact in float32 in any evaluation order
LATTICE_ON = ((3, 0, 0), (2, 2, 1), (-1, -2, -2), (0, 0, -3))     # d2 == 9 == radius2: in neither mask
LATTICE_INSIDE = (2, 2, 0)                                         # d2 = 8
LATTICE_OUTSIDE = (2, 2, 2)                                        # d2 = 12


def lattice_points():
    """(xyz, refl, centre, radius, want_inside, want_outside): four rows exactly ON the sphere, one inside, one outside, one with a NaN
    coordinate (in neither mask) and one with a +inf coordinate (outside)."""
    c = np.asarray(LATTICE_CENTRE)
    rows = [c + np.asarray(o, dtype=np.float64) for o in LATTICE_ON + (LATTICE_INSIDE, LATTICE_OUTSIDE)]
    rows.append(np.asarray([np.nan, 2.0, 3.0]))
    rows.append(np.asarray([1.0, np.inf, 3.0]))
    xyz = np.asarray(rows, dtype=np.float32)
    want_inside = np.asarray([0, 0, 0, 0, 1, 0, 0, 0], dtype=bool)
    want_outside = np.asarray([0, 0, 0, 0, 0, 1, 0, 1], dtype=bool)
    refl = np.linspace(0.1, 0.8, len(rows)).astype(np.float32)
    return xyz, refl, LATTICE_CENTRE, LATTICE_RADIUS, want_inside, want_outside
