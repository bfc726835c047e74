"""The float64 restatement of include/gsr_hip_unbounded.h (tests/unbounded_ref.py) against what is known without it: the contraction and
its inverse, the continuity at the unit sphere, the zero crossing of a sphere that lies in the shell, and the conditions that keep the
GPU tests' comparisons (tests/test_gpu_unbounded.py) from passing on nothing.  No GPU."""
import itertools

import numpy as np
import pytest

import mesh_ref as M
import unbounded_ref as U


def test_contract_and_uncontract_invert_each_other():
    rs = np.random.RandomState(0)
    d = rs.randn(4000, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = np.concatenate([np.linspace(1e-6, 1.99, 3000), [1.0, 1.0 - 1e-12, 1.0 + 1e-12], rs.uniform(0, 1.99, 997)])
    y = d * m[:, None]
    x = U.uncontract(y)
    assert np.abs(U.contract(x) - y).max() <= 1e-12
    assert np.abs(np.linalg.norm(U.contract(x), axis=1) - U.contract_norm(np.linalg.norm(x, axis=1))).max() <= 1e-12
    # and the other way round, from world points out to a norm of 100 (1 / (2 - 1.99))
    X = d * np.concatenate([np.linspace(1e-6, 100, 3000), rs.uniform(0, 100, 1000)])[:, None]
    assert (np.abs(U.uncontract(U.contract(X)) - X) / np.maximum(1, np.abs(X))).max() <= 1e-12
    assert np.linalg.norm(U.contract(X), axis=1).max() < 2


def test_position_and_truncation_are_continuous_at_the_unit_sphere():
    voxel = 0.01
    for eps in (1e-3, 1e-6, 1e-9):
        lo, hi = np.array([[0.0, 1.0 - eps, 0.0]]), np.array([[0.0, 1.0 + eps, 0.0]])
        assert np.abs(U.uncontract(hi) - U.uncontract(lo)).max() <= 2.5 * eps
        assert abs(float(U.trunc_of(1 + eps, voxel)) - float(U.trunc_of(1 - eps, voxel))) <= 5 * voxel * 1.01 * eps
    assert float(U.trunc_of(1.0, voxel)) == 5 * voxel == float(U.trunc_of(0.2, voxel))
    assert float(U.trunc_of(1.95, voxel)) == float(U.trunc_of(1.9, voxel)) == pytest.approx(50 * voxel)
    m = np.linspace(0, 1.999, 500)
    assert (np.diff(U.trunc_of(m, voxel)) >= 0).all() and (np.diff(m * U.uncontract_scale(m)) > 0).all()


def test_uncontract_points_beyond_the_shell_are_finite_and_clipped():
    src = np.array([[0.1, -0.2, 0.3], [1.2, 0.0, 0.9], [2.0, 0.0, 0.0], [3.0, -4.0, 1.0], [0.0, 0.0, 1.999]], np.float32)
    out = U.uncontract_points(src, (0.5, 0.0, -0.5), 2.0, 32.0)
    assert np.isfinite(out).all() and np.abs(out).max() <= 32.0
    assert np.array_equal(out[0], np.array([0.5, 0.0, -0.5]) + 2.0 * src[0].astype(np.float64))
    assert out[2, 0] == 32.0 and out[3, 1] == -32.0 and out[4, 2] == 32.0
    assert np.allclose(out[1], np.array([0.5, 0.0, -0.5]) + 2.0 * U.uncontract(src[1].astype(np.float64)))


# ------------------------------------------------------------------------------------------------- a known answer
KA_CENTRE, KA_RADIUS, KA_RHO, KA_N, KA_EXTENT, KA_ROUNDS = (0.3, -0.1, 0.2), 0.5, 1.0, 33, 1.9, 8


@pytest.fixture(scope="module")
def sphere_views():
    views = []
    for cam in U.axis_cameras(121, 121, KA_CENTRE, 4.0, fov_deg=60.0):
        depth = M.ray_depth_map(cam, KA_CENTRE, KA_RHO, np.array([0.0, 0.0, 1.0]), 1e9)
        depth[depth > 100] = 0
        views.append((cam, depth))
    return views


def _crossing(lat, direction):
    """The contracted radius of the outermost sign change of tsdf along the lattice line from the centre node in `direction`, linearly
    interpolated; None without one."""
    mid, a = lat.n // 2, lat.axis()
    at = [(mid + s * direction[2], mid + s * direction[1], mid + s * direction[0]) for s in range(mid + 1)]
    v = np.array([lat.tsdf[i] for i in at])
    r = np.array([np.linalg.norm([a[i[2]], a[i[1]], a[i[0]]]) for i in at])
    changes = [s for s in range(len(v) - 1) if (v[s] < 0) != (v[s + 1] < 0)]
    if not changes:
        return None
    s = changes[-1]
    return r[s] + (r[s + 1] - r[s]) * v[s] / (v[s] - v[s + 1])


def test_a_sphere_in_the_shell_crosses_zero_at_its_contracted_radius(sphere_views):
    """A sphere of world radius 1 about the centre of a contraction of radius 0.5 lies at the contracted radius 2 - 1 / 2 = 1.5.  Seen by
    the six axis cameras, the fused field crosses zero there to half a lattice step, along the six axes (one camera sees the crossing)
    and the eight body diagonals (three do).

    The fresh volume's tsdf = 1 at weight 1 counts as one observation of free space, so a node that k fusions have seen at the truncated
    distance t holds (1 + k t) / (1 + k) and changes sign at sdf = -trunc / k, not at 0: upstream's state, made for captures of hundreds
    of frames.  The six views are therefore fused KA_ROUNDS times each, as a capture that keeps revisiting them; test_one_fusion...
    below pins the other end.  (Along the face diagonals this lattice has no node inside the truncation band: 33 nodes over 3.8 units
    put neighbours on a diagonal further apart than the band is deep.)"""
    lat = U.Lattice(KA_N, KA_EXTENT, KA_CENTRE, KA_RADIUS)
    assert lat.axis()[KA_N // 2] == 0.0                                   # the lattice has a centre node
    for _ in range(KA_ROUNDS):
        for cam, depth in sphere_views:
            U.integrate(lat, depth, cam["viewmatrix"], cam["projmatrix"])
    want = float(U.contract_norm(KA_RHO / KA_RADIUS))
    assert want == 1.5
    directions = [d for d in itertools.product((-1, 0, 1), repeat=3) if sum(map(abs, d)) in (1, 3)]
    assert len(directions) == 14
    for d in directions:
        got = _crossing(lat, d)
        assert got is not None, d
        print(d, f"crossing at {got:.4f}, {(got - want) / lat.step:+.3f} lattice steps from {want}")
        assert abs(got - want) <= 0.5 * lat.step, (d, got)


def test_one_fusion_of_one_view_leaves_no_node_inside(sphere_views):
    """t > -1 for every node a view writes (sdf > -trunc), so after one fusion tsdf = (1 + t) / 2 > 0 everywhere: the first observation
    cannot outweigh the fresh state."""
    lat = U.Lattice(KA_N, KA_EXTENT, KA_CENTRE, KA_RADIUS)
    cam, depth = sphere_views[0]
    written, _ = U.integrate(lat, depth, cam["viewmatrix"], cam["projmatrix"])
    assert written.sum() > 500 and (lat.tsdf > 0).all() and lat.tsdf[written].min() < 0.2
    assert (lat.weight[written] == 2).all() and (lat.weight[~written] == 1).all() and (lat.tsdf[~written] == 1).all()


# ------------------------------------------------------------------------------------------------- the fixture's conditions
@pytest.fixture(scope="module")
def fixture_views():
    return M.integrate_fixture()


@pytest.mark.parametrize("n, extent", U.FIX_LATTICES)
def test_fixture_reaches_what_the_gpu_tests_compare(fixture_views, n, extent):
    ref = U.fixture_reference(n, extent, fixture_views)
    lat = U.Lattice(n, extent, U.FIX_CENTRE, U.FIX_RADIUS)
    m = np.linalg.norm(lat.nodes(), axis=-1)
    zones = dict(ball=int((m < 1).sum()), shell=int(((m >= 1) & (m < 2)).sum()), beyond=int((m >= 2).sum()))
    written = [r[2] for r in ref]
    any_view, all_views = written[0] | written[1] | written[2], written[0] & written[1] & written[2]
    tsdf, weight, _, unstable = ref[-1]
    print(f"n {n} extent {extent}: {zones}, written {int(any_view.sum())}, by all three {int(all_views.sum())}, inside {int((tsdf < 0).sum())}, "
          f"unstable {int(unstable.sum())}")
    assert unstable.sum() <= 0.01 * n ** 3
    assert any_view.sum() >= 3000 and (tsdf < 0).sum() >= 200 and all_views.sum() >= 400
    assert min(zones.values()) > 0
    # written nodes lie in the ball and in the shell, none beyond; the weights count the views
    assert (any_view & (m < 1)).sum() > 100 and (any_view & (m >= 1)).sum() > 100 and not (any_view & (m >= 2)).any()
    assert np.array_equal(weight, 1.0 + written[0] + written[1] + written[2])
    if (n, extent) == (33, 1.9):
        assert zones == dict(ball=2517, shell=17488, beyond=15932)


def test_fixture_points_are_seen_and_coloured(fixture_views):
    pts = U.fixture_points()
    color, weight = np.zeros((len(pts), 3)), np.zeros(len(pts))
    unstable = np.zeros(len(pts), bool)
    for vw in fixture_views:
        _, uns = U.fuse_points(pts, color, weight, vw["depth"], vw["rgb"], vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"], 0.15)
        unstable |= uns
    print(f"points by views that saw them: {np.bincount(weight.astype(int), minlength=4).tolist()}, unstable {int(unstable.sum())}")
    assert unstable.sum() <= 0.01 * len(pts)
    assert (weight == 0).sum() > 200 and (weight >= 1).sum() > 1500 and (weight == 3).sum() > 100
    assert (color[weight == 0] == 0).all() and color[weight > 0].min() > 0 and color.max() < 1
