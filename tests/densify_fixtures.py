"""Seeded inputs of the densification-plan tests (tests/test_gpu_densify_plan.py, tests/densify_plan_timing.py): a scene of gsr_synth, the
statistics and scale draws of tests/test_gpu_densify.py (a few hundred training views: some points never seen, some of low blend weight,
a spread of sizes around percent_dense * extent with some huge), the noise of the split, and hand-made class mixes.  numpy only; not a
conftest: tests import it.

Why the GPU tests may ask for BIT equality of plan="device" with plan="torch".  The weight and gradient tests are IEEE divisions and
compares of identical float32 inputs: they agree exactly and need no margin.  The tests that pass through expf (the largest scale against
dense_limit, 0.1 extent, 1.5 extent) or a three-term sum (the squared distance against extent^2) can differ between torch's kernels and
the library's by a few ulp (1 ulp = 6e-8 relative; expf and a contracted sum: under 1e-6).  So every fixture is kept clear of those
thresholds: `bands(fx)` evaluates every row and every child of the split (children in float64 after oracle_densify, with the noise the
test uses) and returns those whose largest scale lies within BAND = 1e-5 relative of a limit or whose squared distance lies within BAND
of extent^2; `make` moves such a row off by a factor of 1.0001 (a row is never dropped) until none is left.
tests/test_densify_fixtures.py asserts on the CPU that the bands are empty for every fixture the GPU tests use."""
import numpy as np

BAND = 1e-5
NUDGE = 1.0001
MAX_GRAD, MIN_OPACITY, PERCENT_DENSE, MIN_WEIGHT = 0.0002, 0.05, 0.01, 0.01
EXTENT = 3.0
MEAN = (0.25, -0.5, 4.0)
N_CHILDREN = 2
STAT_NAMES = ("xyz_gradient_accum", "denom", "accum_w", "denom_w", "max_radii2D")
GROUPS = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")
F32 = np.float32


def limits(extent=EXTENT):
    """The thresholds as the plans compare against them: computed in double, rounded to float32 once."""
    return dict(dense=F32(PERCENT_DENSE * extent), near=F32(0.1 * extent), far=F32(1.5 * extent), extent2=F32(extent ** 2))


def classes(fx):
    """(pruned, clone, parent, m): the class of every old row.  Weight and gradient in float32 (IEEE, what both plans compute), the largest
    scale m in float64 from the float32 log-scales."""
    s = fx["stats"]
    lim = limits(fx["extent"])
    with np.errstate(all="ignore"):
        w = s["accum_w"] / s["denom_w"]
        w[s["denom_w"] == 0] = 0
        g = s["xyz_gradient_accum"] / s["denom"]
    g[np.isnan(g)] = 0
    pruned = w < F32(MIN_WEIGHT)
    m = np.exp(fx["scene"]["scales"].astype(np.float64)).max(1)
    clone = ~pruned & (np.abs(g) >= F32(MAX_GRAD)) & (m <= lim["dense"])
    parent = ~pruned & (g >= F32(MAX_GRAD)) & (m > lim["dense"])
    return pruned, clone, parent, m


def children(fx, parent):
    """(parent row of child j, child_xyz, largest child scale) in float64, after oracle_densify.Model.densify_and_split."""
    from oracle import oracle_densify as od
    N, sc = fx["N"], fx["scene"]
    idx = np.nonzero(parent)[0]
    par = np.tile(idx, N)
    if par.size == 0:
        return par, np.zeros((0, 3)), np.zeros(0)
    s = np.exp(sc["scales"][par].astype(np.float64))
    noise = fx["noise_pool"][:par.size].astype(np.float64)
    smp = np.concatenate([s * noise, np.zeros((par.size, 3 - s.shape[1]))], -1)
    R = od.build_rotation(sc["rotations"][par].astype(np.float64))
    xyz = np.einsum("nij,nj->ni", R, smp) + sc["means3D"][par].astype(np.float64)
    return par, xyz, (s / (0.8 * N)).max(1)


def _near(v, limit):
    return np.abs(v / np.float64(limit) - 1.0) < BAND


def bands(fx):
    """(rows whose largest scale, or a child's, lies in a band; rows whose squared distance, or a child's, does; +1 / -1 per row of the
    first list: the side of the limit the row's own scale lies on, +1 for a row listed for its child)."""
    lim = limits(fx["extent"])
    mean = np.asarray(fx["mean"], np.float64)
    pruned, clone, parent, m = classes(fx)
    par, cxyz, cm = children(fx, parent)
    d2 = ((fx["scene"]["means3D"].astype(np.float64) - mean) ** 2).sum(-1)
    cd2 = ((cxyz - mean) ** 2).sum(-1)
    own = np.zeros(m.size, bool)
    side = np.ones(m.size)
    for L in (lim["dense"], lim["near"], lim["far"]):
        hit = _near(m, L)
        own |= hit
        side[hit & (m < np.float64(L))] = -1.0
    child_hit = np.zeros(m.size, bool)
    for L in (lim["dense"], lim["near"], lim["far"]):
        child_hit[par[_near(cm, L)]] = True
    side[child_hit & ~own] = 1.0
    bad_scale = np.nonzero(own | child_hit)[0]
    bad_d2 = _near(d2, lim["extent2"])
    bad_d2[par[_near(cd2, lim["extent2"])]] = True
    return bad_scale, np.nonzero(bad_d2)[0], side[bad_scale]


def clear_bands(fx):
    """Moves the rows `bands` lists off their thresholds by a factor of 1.0001 (the scale of the row; its offset from the mean) until none
    is left.  Returns the number of rows moved."""
    moved = 0
    sc = fx["scene"]
    mean = np.asarray(fx["mean"], F32)
    for _ in range(50):
        bad_scale, bad_d2, side = bands(fx)
        if bad_scale.size == 0 and bad_d2.size == 0:
            return moved
        moved += bad_scale.size + bad_d2.size
        sc["scales"][bad_scale] += (side * np.log(NUDGE)).astype(F32)[:, None]
        sc["means3D"][bad_d2] = mean + (sc["means3D"][bad_d2] - mean) * F32(NUDGE)
    raise AssertionError("rows stay inside a band after 50 rounds")


def summary(fx):
    """Counts by class, and the rows the last prune drops (float64, as oracle_densify judges them)."""
    lim = limits(fx["extent"])
    mean = np.asarray(fx["mean"], np.float64)
    pruned, clone, parent, m = classes(fx)
    par, cxyz, cm = children(fx, parent)

    def big(mm, xyz):
        inside = ((xyz - mean) ** 2).sum(-1) < np.float64(lim["extent2"])
        return np.where(inside, mm > lim["near"], mm > lim["far"])
    stay = ~pruned & ~parent
    big_rows = big(m, fx["scene"]["means3D"].astype(np.float64))
    return dict(pruned=int(pruned.sum()), cloned=int(clone.sum()), split=int(parent.sum()), kept=int((stay & ~clone).sum()),
                big=int((stay & big_rows).sum() + (clone & big_rows).sum() + big(cm, cxyz).sum()),
                length=int(stay.sum() + clone.sum() + par.size))


def make(P, seed, mix="views", stats_seed=3, mu=-3.2, extent=EXTENT, mean=MEAN, N=N_CHILDREN):
    """A fixture: dict(P, N, extent, mean, scene (gsr_synth.make_scene, with LOG-scales under "scales"), stats (the five float32 rows),
    noise_pool ([N P, 2] standard normal: the split of k parents uses its first N k rows)).  mix:
      "views"      the statistics and scale draws of tests/test_gpu_densify.py; row 0 is made a plain survivor (a small P keeps a row)
      "denoms"     "views" with rows of every kind of zero denominator set by hand (see the code)
      "identity"   nothing selected, nothing pruned
      "clones"     every row a clone
      "parents"    every row but five a parent so large that each child is dropped as big; the five are small plain survivors
      "one"        every row but one pruned by weight"""
    import gsr_synth as S
    sc = S.make_scene(P, "S", seed=seed, mu=mu)
    rs = np.random.RandomState(stats_seed)
    denom = rs.randint(0, 5, P).astype(F32)
    gacc = (rs.rand(P) * 8e-4 * denom).astype(F32)
    dw = rs.randint(0, 4, P).astype(F32)
    aw = (rs.rand(P) * 0.05 * dw).astype(F32)
    radii = rs.randint(0, 60, P).astype(F32)
    log_scales = np.log(np.exp(rs.randn(P, 2) * 1.2) * 0.03).astype(F32)
    noise_pool = rs.randn(N * P, 2).astype(F32)
    one, zero = np.ones(P, F32), np.zeros(P, F32)
    small = np.log(0.004 + 0.01 * rs.rand(P, 2)).astype(F32)            # largest scale <= 0.014 < dense_limit = 0.03
    if mix in ("views", "denoms"):
        denom[0], gacc[0], dw[0], aw[0], log_scales[0] = 1, 0, 1, 1, small[0]
    if mix == "denoms" and P >= 64:
        r = np.arange(8, 56)
        dw[r], aw[r] = 1, 1                                               # they survive the weight prune ...
        denom[r[:16]], gacc[r[:16]] = 0, 0                                # 0 / 0 = NaN -> 0: not selected (small: the last prune keeps them)
        log_scales[r[:16]] = small[r[:16]]
        denom[r[16:32]], gacc[r[16:32]] = 0, 1e-3                         # x / 0 = inf: selected, as torch does
        log_scales[r[16:24]] = small[r[16:24]]                            #   ... eight of them clones, eight parents
        log_scales[r[24:32]] = np.log(0.05)
        dw[r[32:]], aw[r[32:]] = 0, 1                                     # denom_w == 0: pruned whatever accum_w holds
    elif mix == "identity":
        denom, gacc, dw, aw = one.copy(), zero.copy(), one.copy(), one.copy()
    elif mix == "clones":
        denom, gacc, dw, aw, log_scales = one.copy(), one.copy(), one.copy(), one.copy(), small
    elif mix == "parents":
        denom, gacc, dw, aw = one.copy(), one.copy(), one.copy(), one.copy()
        log_scales = np.log(20.0 + rs.rand(P, 2)).astype(F32)             # children: 12.5 and more > 1.5 extent: dropped wherever they land
        few = np.arange(5) * (P // 5) + 3
        gacc[few], log_scales[few] = 0, small[few]
    elif mix == "one":
        denom, gacc, dw, aw = one.copy(), zero.copy(), one.copy(), zero.copy()
        aw[P // 2 + 1], log_scales[P // 2 + 1] = 1, small[P // 2 + 1]     # (small: the last prune keeps it)
    elif mix not in ("views", "denoms"):
        raise ValueError(mix)
    scene = {k: np.array(sc[k], F32) for k in GROUPS}
    scene["scales"] = log_scales
    fx = dict(P=P, N=N, extent=extent, mean=tuple(float(v) for v in mean), mix=mix, scene=scene, noise_pool=noise_pool,
              stats=dict(xyz_gradient_accum=gacc, denom=denom, accum_w=aw, denom_w=dw, max_radii2D=radii))
    fx["moved"] = clear_bands(fx)
    return fx


ROWS_PER_WORKGROUP = 256            # PLAN_B of csrc/gsr_densify.hip: the rows a workgroup of the classify kernels ranks
SCAN_CHUNK_ROWS = 256 * ROWS_PER_WORKGROUP      # the count scan takes 256 workgroups per turn: 65536 rows

# (P, scene seed, mix, statistics seed) of every fixture the GPU tests use
MAIN = (30000, 7, "views", 3)
SHARDED = (9001, 11, "views", 5)
SMALL = [(P, 20 + i, "views", 40 + i) for i, P in enumerate(
    (1, 2, 63, 64, 65, ROWS_PER_WORKGROUP - 1, ROWS_PER_WORKGROUP, ROWS_PER_WORKGROUP + 1, 2 * ROWS_PER_WORKGROUP + 1, SCAN_CHUNK_ROWS + 1))]
MIXES = [(300, 31, mix, 9) for mix in ("identity", "clones", "parents", "one")]
DENOMS = (2000, 33, "denoms", 13)
ALL = [MAIN, SHARDED] + SMALL + MIXES + [DENOMS]

_cache = {}


def get(key):
    """make(*key), computed once per process and handed out as it is: callers copy what they change."""
    if key not in _cache:
        _cache[key] = make(key[0], key[1], mix=key[2], stats_seed=key[3])
    return _cache[key]
