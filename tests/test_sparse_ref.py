"""The float64 restatement of include/gsr_hip_sparse.h (tests/sparse_ref.py) against what is known without it, on the CPU: the blocks the
touch rule selects on the fusion fixture at three voxel sizes, that the surface over those blocks is the dense volume's (the argument in
the header), and the allocation order."""
import numpy as np
import pytest

import mesh_ref as M
import sparse_ref as R

# (dims, voxel, sdf_trunc, blocks selected, blocks of the box, nV, nT): the three views of mesh_ref.integrate_fixture() with colour and alpha
TABLE = (((23, 19, 17), 0.1, 0.25, 18, 27, 432, 694),
         ((45, 37, 33), 0.05, 0.1, 41, 150, 1966, 3452),
         ((67, 55, 49), np.float32(1.0 / 30.0), 0.1, 83, 441, 4709, 8670))


@pytest.fixture(scope="module")
def views():
    return M.integrate_fixture()


def two_phase(views, dims, voxel, sdf_trunc):
    """(sparse volume, dense volume) after every view was touched, the blocks allocated once, and every view fused into both."""
    vol, dense = R.Volume(dims, M.FIX_ORIGIN, voxel), M.Volume(dims, M.FIX_ORIGIN, voxel)
    for vw in views:
        sure, possible = vol.touch(vw, M.FIX_ALPHA_MIN, sdf_trunc, M.FIX_DEPTH_TRUNC)
        assert set(sure) <= set(possible)
    vol.allocate()
    for vw in views:
        vol.integrate(vw, M.FIX_ALPHA_MIN, sdf_trunc, M.FIX_DEPTH_TRUNC)
        M.integrate(dense, vw["depth"], vw["rgb"], vw["alpha"], M.FIX_ALPHA_MIN, vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"], sdf_trunc,
                    M.FIX_DEPTH_TRUNC)
    return vol, dense


@pytest.mark.parametrize("dims, voxel, sdf_trunc, selected, of, nV, nT", TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_the_surface_over_the_selected_blocks_is_the_dense_one(views, dims, voxel, sdf_trunc, selected, of, nV, nT):
    vol, dense = two_phase(views, dims, voxel, sdf_trunc)
    assert (vol.blocks, int(np.prod(R.grid(dims)))) == (selected, of)
    assert (np.diff(vol.block_of_slot[:vol.blocks]) > 0).all()                  # one allocation: slots ascend with the block index
    # allocated nodes hold the dense values, bit for bit: every view was touched before any was fused
    tsdf, weight, color, has = vol.to_dense()
    assert (tsdf[has] == dense.tsdf[has]).all() and (weight[has] == dense.weight[has]).all() and (color[:, has] == dense.color[:, has]).all()
    f32 = lambda a: a.astype(np.float32)
    # the dense extraction, and the dense extraction of the planes masked to the selected blocks: identical
    full = M.extract(f32(dense.tsdf), f32(dense.weight), f32(dense.color), M.FIX_ORIGIN, voxel)
    masked = M.extract(f32(tsdf), f32(weight), f32(color), M.FIX_ORIGIN, voxel)
    assert (len(full[0]), len(full[2])) == (nV, nT)
    for a, b in zip(full, masked):
        assert np.array_equal(a, b)
    # the restatement in pool order is that mesh, permuted
    V, C, F, keys, face_cells, _ = R.extract_volume(vol)
    Vp, Cp, Fp = R.to_pool_order(masked, R.dense_keys(f32(tsdf), f32(weight)), keys, face_cells)
    assert np.array_equal(V, Vp) and np.array_equal(C, Cp) and np.array_equal(F, Fp)
    if dims == (67, 55, 49):
        valid = dense.weight >= 1
        assert 5e-4 < np.abs(dense.tsdf[valid]).min() < 6e-4                     # no sign of the fixture hangs on the device's rounding


def test_touch_bounds_coincide_on_the_fixture(views):
    """At S = (67, 55, 49) no unstable node changes a block: per view the sure and the possible sets are the same (72, 18 and 55 blocks)."""
    dims, voxel, sdf_trunc = TABLE[2][:3]
    counts = []
    for vw in views:
        sure, possible = R.touch(dims, M.FIX_ORIGIN, voxel, vw["depth"], vw["alpha"], M.FIX_ALPHA_MIN, vw["cam"]["viewmatrix"],
                                 vw["cam"]["projmatrix"], sdf_trunc, M.FIX_DEPTH_TRUNC)
        assert np.array_equal(sure, possible)
        counts.append(len(sure))
    assert counts == [72, 18, 55]


def test_a_near_tie_is_evaluated_under_each_candidate_pixel():
    """One node whose pixel coordinate is a half-integer: band under the pixel on one side, far outside it under the other.  It is
    possible, not sure; with both pixels inside the band it still is not sure (the decision is unstable) but changes no set."""
    import cameras
    cam = cameras.family("offcentre", M.FIX_W, M.FIX_H, 20)
    dims, voxel = (2, 2, 2), 1e-6                          # eight nodes within 1e-4 of a pixel of one another: all at the tie
    # find the pixel the node at `origin` projects to, then move the origin so that px sits on the half-integer
    V, P = cam["viewmatrix"].astype(np.float64).reshape(-1), cam["projmatrix"].astype(np.float64).reshape(-1)

    def project(x):
        pw = P[3] * x[0] + P[7] * x[1] + P[11] * x[2] + P[15]
        px = ((P[0] * x[0] + P[4] * x[1] + P[8] * x[2] + P[12]) / pw + 1) * M.FIX_W / 2 - 0.5
        return px, V[2] * x[0] + V[6] * x[1] + V[10] * x[2] + V[14]
    x = np.array([-0.2, 0.1, 0.8])
    for _ in range(40):                                    # Newton on px(x0) = 30.5
        px, _ = project(x)
        slope = (project(x + np.array([1e-6, 0, 0]))[0] - px) / 1e-6
        x[0] -= (px - 30.5) / slope
    x = x.astype(np.float32)
    px, z = project(x.astype(np.float64))
    assert abs(px - 30.5) < 2e-4
    depth = np.zeros((M.FIX_H, M.FIX_W), np.float32)
    py = int(round(((P[1] * x[0] + P[5] * x[1] + P[9] * x[2] + P[13]) / (P[3] * x[0] + P[7] * x[1] + P[11] * x[2] + P[15]) + 1) * M.FIX_H / 2 - 0.5))
    depth[py - 1:py + 2, 30], depth[py - 1:py + 2, 31] = z, z + 0.9
    args = (None, 0.5, cam["viewmatrix"], cam["projmatrix"], 0.1, 3.0)
    sure, possible = R.touch(dims, x, voxel, depth, *args)
    assert len(sure) == 0 and list(possible) == [0]
    depth[:, 31] = depth[:, 30]
    sure, possible = R.touch(dims, x, voxel, depth, *args)
    assert list(possible) == [0]


def test_allocation_gives_the_lowest_blocks_first_and_continues_after_growth():
    table = np.full(40, R.UNTOUCHED, np.int32)
    waiting = [3, 7, 8, 21, 39]
    table[waiting] = R.WAITING
    block_of_slot = np.full(3, -9, np.int32)
    counts = R.allocate(table, block_of_slot, 3, (0, 0))
    assert counts == (3, 5) and list(block_of_slot) == [3, 7, 8]
    assert [int(table[b]) for b in waiting] == [0, 1, 2, R.WAITING, R.WAITING]
    # a second call at the same capacity changes nothing
    assert R.allocate(table, block_of_slot, 3, counts) == (3, 5) and list(block_of_slot) == [3, 7, 8]
    # growth: the old slots are kept and the call continues behind them
    grown = np.concatenate([block_of_slot, np.full(3, -9, np.int32)])
    table[12] = R.WAITING                                  # touched in between: allocated behind the old slots, although its index is lower
    counts = R.allocate(table, grown, 6, (3, 5))
    assert counts == (6, 6) and list(grown) == [3, 7, 8, 12, 21, 39]
    assert [int(table[b]) for b in (3, 7, 8, 12, 21, 39)] == [0, 1, 2, 3, 4, 5]
    assert (np.delete(table, [3, 7, 8, 12, 21, 39]) == R.UNTOUCHED).all()
    # capacity 0: nothing is written, everything is wanted
    fresh = np.full(10, R.WAITING, np.int32)
    assert R.allocate(fresh, np.zeros(0, np.int32), 0, (0, 0)) == (0, 10) and (fresh == R.WAITING).all()
