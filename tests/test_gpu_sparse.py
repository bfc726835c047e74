"""gsr_mesh.SparseTSDFVolume on the GPU against the float64 restatement (tests/sparse_ref.py, on top of tests/mesh_ref.py): which blocks a
view touches, the allocation order, the fusion into the pool (and that nothing else is written), the extraction in pool order, the dense
device path on the same views, stream ordering, and GaussianExtractor.extract_mesh_bounded(sparse=True) end to end.

The main fixture S is mesh_ref's fusion fixture refined to 67 x 55 x 49 nodes (voxel float32(1/30), sdf_trunc 0.1): 9 x 7 x 7 blocks whose
edge blocks are 3, 7 and 1 node thick, 83 of them in the band of the three views.

Tolerances.  Fusion: the project's INTEGRATE_TOL (tests/test_gpu_mesh.py: four times the largest |device - restatement| observed on an
MI355X for the dense kernel, whose arithmetic the sparse kernel repeats), restated here.  Extraction: counts and faces exactly, positions
and colours within mesh_ref.extract_bounds(), which follows from the emit kernel's arithmetic.
"""
import numpy as np
import pytest
import torch

import cameras
import mesh_ref as M
import poison
import sparse_ref as R

pytestmark = pytest.mark.gpu

INTEGRATE_TOL = {"tsdf": 4 * 3.18e-7, "color": 4 * 5.97e-8}
S_DIMS, S_VOXEL, S_TRUNC = (67, 55, 49), np.float32(1.0 / 30.0), 0.1
S_BLOCKS, ANISO_BLOCKS = 83, 55
GUARD = 64                       # floats in front of and behind each guarded plane
SPARE = 5                        # slots of the poisoned pool beyond n_slots
ROW_GUARD = 16                   # rows behind verts, colours and faces


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _volume(dims=S_DIMS, origin=M.FIX_ORIGIN, voxel=S_VOXEL, color=True):
    import gsr_mesh
    return gsr_mesh.SparseTSDFVolume(origin, voxel, dims, "cuda", color=color)


def _stage(vw, color=True, alpha=True):
    """The view's inputs on the device: (depth, camera object, rgb | None, alpha | None)."""
    return (_dev(vw["depth"]), cameras.view_of(vw["cam"]), _dev(vw["rgb"]) if color else None, _dev(vw["alpha"]) if alpha else None)


FIX = dict(alpha_min=M.FIX_ALPHA_MIN, sdf_trunc=S_TRUNC, depth_trunc=M.FIX_DEPTH_TRUNC)


def _touch(vol, staged):
    depth, cam, _, alpha = staged
    vol.touch(depth, cam, alpha=alpha, **FIX)


def _integrate(vol, staged):
    depth, cam, rgb, alpha = staged
    vol.integrate(depth, cam, rgb=rgb, alpha=alpha, **FIX)


def _two_phase(vol, staged_views):
    for st in staged_views:
        _touch(vol, st)
    vol.allocate()
    for st in staged_views:
        _integrate(vol, st)
    return vol


def _positions(table, n_slots, dims):
    """(has, slot, local), each [nz, ny, nx]: whether a node of the box has storage, and where in the pool."""
    shell = R.Volume(dims, (0, 0, 0), 1.0, color=False)
    shell.table, shell.counts = np.asarray(table), (n_slots, n_slots)
    slot, local = shell._index()
    return slot >= 0, slot, local


@pytest.fixture(scope="module")
def views():
    return M.integrate_fixture()


@pytest.fixture(scope="module")
def touched_ref(views):
    """[(sure, possible)] per view of S."""
    return [R.touch(S_DIMS, M.FIX_ORIGIN, S_VOXEL, vw["depth"], vw["alpha"], M.FIX_ALPHA_MIN, vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"], S_TRUNC,
                    M.FIX_DEPTH_TRUNC) for vw in views]


def _restate(views, color=True, alpha=True):
    """The two-phase restatement over S: (volume, [(tsdf, weight, color | None pool planes, written, unstable so far) after each view])."""
    ref = R.Volume(S_DIMS, M.FIX_ORIGIN, S_VOXEL, color=color)
    for vw in views:
        sure, possible = ref.touch(vw, M.FIX_ALPHA_MIN, S_TRUNC, M.FIX_DEPTH_TRUNC, alpha=alpha)
        assert np.array_equal(sure, possible)                     # no unstable node decides a block of S: the device's allocation is this one
    ref.allocate()
    unstable, out = np.zeros(S_DIMS[::-1], bool), []
    for vw in views:
        written, uns, _ = ref.integrate(vw, M.FIX_ALPHA_MIN, S_TRUNC, M.FIX_DEPTH_TRUNC, color=color, alpha=alpha)
        unstable = unstable | uns
        out.append((ref.tsdf.copy(), ref.weight.copy(), None if ref.color is None else ref.color.copy(), written, unstable.copy()))
    return ref, out


@pytest.fixture(scope="module")
def reference(views):
    return _restate(views)


# ------------------------------------------------------------------------------------------------- touch
@pytest.mark.parametrize("n", range(3), ids=[name for name, _ in M.FIX_VIEWS])
def test_touch_lies_between_the_sure_and_the_possible_blocks(views, touched_ref, n):
    sure, possible = touched_ref[n]
    vol, staged = _volume(), _stage(views[n])
    _touch(vol, staged)
    table = vol.table.cpu().numpy()
    touched = np.nonzero(table == R.WAITING)[0]
    assert ((table == R.WAITING) | (table == R.UNTOUCHED)).all()
    print(f"{M.FIX_VIEWS[n][0]}: sure {len(sure)} touched {len(touched)} possible {len(possible)} of {len(table)}")
    assert set(sure) <= set(touched) <= set(possible)
    if M.FIX_VIEWS[n][0] == "aniso":
        assert np.array_equal(sure, possible) and len(sure) == ANISO_BLOCKS and np.array_equal(touched, sure)
    _touch(vol, staged)                                            # a second touch of the same view changes nothing
    assert np.array_equal(vol.table.cpu().numpy(), table)
    assert vol.blocks == 0 and vol.capacity == 0 and vol.counts.tolist() == [0, 0]


def test_touch_leaves_a_block_with_a_slot_alone(views, touched_ref):
    vol = _volume()
    _touch(vol, _stage(views[2]))
    assert vol.allocate() == ANISO_BLOCKS
    before = vol.table.cpu().numpy()
    for vw in views:
        _touch(vol, _stage(vw))
    after = vol.table.cpu().numpy()
    had = before >= 0
    assert had.sum() == ANISO_BLOCKS and np.array_equal(after[had], before[had])
    every = np.unique(np.concatenate([s for s, _ in touched_ref]))
    assert np.array_equal(np.nonzero(after != R.UNTOUCHED)[0], every) and (after[~had][after[~had] != R.UNTOUCHED] == R.WAITING).all()


# ------------------------------------------------------------------------------------------------- allocate
def _allocate_raw(table, dims, block_of_slot, capacity, counts):
    from _gsr import check, lib, ptr, stream_ptr
    scratch = torch.empty(int(lib.gsr_sparse_tsdf_allocate_scratch_bytes(*dims)), dtype=torch.uint8, device="cuda")
    scratch.fill_(0xA5)
    check(lib.gsr_sparse_tsdf_allocate(ptr(table), *dims, ptr(block_of_slot), capacity, ptr(counts), ptr(scratch), scratch.numel(), stream_ptr("cuda")),
          "gsr_sparse_tsdf_allocate")


@pytest.fixture(scope="module")
def touched_table(views):
    """The table of S after the three touches, on the host."""
    vol = _volume()
    for vw in views:
        _touch(vol, _stage(vw))
    return vol.table.cpu().numpy()


@pytest.mark.parametrize("capacity", [0, S_BLOCKS - 1, S_BLOCKS], ids=["none", "one-short", "exact"])
def test_allocate_hands_out_slots_in_ascending_block_order(touched_table, capacity):
    waiting = np.nonzero(touched_table == R.WAITING)[0]
    assert len(waiting) == S_BLOCKS
    table, counts = _dev(touched_table, torch.int32), torch.zeros(2, dtype=torch.int64, device="cuda")
    slots = torch.full((capacity + 8,), -7, dtype=torch.int32, device="cuda")
    _allocate_raw(table, S_DIMS, slots if capacity else None, capacity, counts)
    assert counts.tolist() == [capacity, S_BLOCKS]
    got, table = slots.cpu().numpy(), table.cpu().numpy()
    assert np.array_equal(got[:capacity], waiting[:capacity]) and (got[capacity:] == -7).all()
    assert np.array_equal(table[waiting[:capacity]], np.arange(capacity)) and (table[waiting[capacity:]] == R.WAITING).all()
    rest = np.ones(len(table), bool)
    rest[waiting] = False
    assert (table[rest] == R.UNTOUCHED).all()
    # the restatement agrees
    t2, b2 = touched_table.copy(), np.full(capacity, -7, np.int32)
    assert R.allocate(t2, b2, capacity, (0, 0)) == (capacity, S_BLOCKS) and np.array_equal(t2, table) and np.array_equal(b2, got[:capacity])


def test_allocate_in_two_rounds_continues_behind_the_slots_in_use(views, touched_ref):
    vol = _volume()
    _touch(vol, _stage(views[2]))
    assert vol.allocate() == ANISO_BLOCKS and vol.capacity == ANISO_BLOCKS
    first = vol.block_of_slot.cpu().numpy().copy()
    assert np.array_equal(first, touched_ref[2][0])
    marks = torch.arange(ANISO_BLOCKS * 512, dtype=torch.float32, device="cuda").reshape(ANISO_BLOCKS, 512)
    vol.tsdf.copy_(marks)
    vol.color[:, 1].copy_(-marks)
    for vw in views[:2]:
        _touch(vol, _stage(vw))
    assert vol.allocate() == S_BLOCKS and vol.blocks == S_BLOCKS and vol.capacity == S_BLOCKS and vol.counts.tolist() == [S_BLOCKS, S_BLOCKS]
    slots = vol.block_of_slot.cpu().numpy()
    every = np.unique(np.concatenate([s for s, _ in touched_ref]))
    assert np.array_equal(slots[:ANISO_BLOCKS], first) and np.array_equal(slots[ANISO_BLOCKS:], np.setdiff1d(every, first))
    assert np.array_equal(vol.table.cpu().numpy()[slots], np.arange(S_BLOCKS))
    # the pool grew: the old slots were copied, the new ones are zero
    assert torch.equal(vol.tsdf[:ANISO_BLOCKS], marks) and torch.equal(vol.color[:ANISO_BLOCKS, 1], -marks)
    assert float(vol.tsdf[ANISO_BLOCKS:].abs().sum() + vol.weight.abs().sum() + vol.color[ANISO_BLOCKS:].abs().sum() + vol.color[:, 0].abs().sum()) == 0.0
    assert vol.allocate() == S_BLOCKS                             # nothing waits: nothing changes
    assert np.array_equal(vol.block_of_slot.cpu().numpy(), slots)
    assert vol.nbytes == 4 * (vol.table.numel() + S_BLOCKS * (1 + 5 * 512))          # the table; per slot its block index and five planes
    vol.reset()
    assert vol.blocks == 0 and (vol.table == -1).all() and float(vol.tsdf.abs().sum()) == 0.0 and vol.extract().faces.shape == (0, 3)


def test_allocate_over_a_table_longer_than_one_round_of_the_spine():
    """2 x 2 x 2 105 600 nodes: 263 200 blocks, 1029 scan blocks of 256 where scan_spine_kernel takes 1024 per round; three in ten wait,
    some hold slots already, and the capacity ends 1000 short."""
    gz = 263_200
    dims = (2, 2, 8 * gz)
    rs = np.random.RandomState(11)
    u = rs.rand(gz)
    table = np.where(u < 0.3, R.WAITING, R.UNTOUCHED).astype(np.int32)
    held = np.nonzero((u > 0.3) & (u < 0.31))[0]
    table[held] = rs.permutation(len(held))
    wanted = int((table == R.WAITING).sum())
    assert (table[1024 * 256:] == R.WAITING).sum() > 100
    capacity = len(held) + wanted - 1000
    t_ref, b_ref = table.copy(), np.full(capacity, -7, np.int32)
    counts_ref = R.allocate(t_ref, b_ref, capacity, (len(held), len(held)))
    assert counts_ref == (capacity, len(held) + wanted)
    t_dev, slots = _dev(table, torch.int32), torch.full((capacity,), -7, dtype=torch.int32, device="cuda")
    counts = torch.tensor([len(held), len(held)], dtype=torch.int64, device="cuda")
    _allocate_raw(t_dev, dims, slots, capacity, counts)
    assert tuple(counts.tolist()) == counts_ref
    assert np.array_equal(t_dev.cpu().numpy(), t_ref) and np.array_equal(slots.cpu().numpy(), b_ref)


# ------------------------------------------------------------------------------------------------- integrate
def _pool_errors(vol, ref, state):
    """Largest |device - restatement| of tsdf and colour over the allocated stable nodes, and whether weight is exact there."""
    tsdf, weight, color, _, unstable = state
    has, slot, local = _positions(ref.table, ref.blocks, S_DIMS)
    at = has & ~unstable
    s, l = slot[at], local[at]
    got_t, got_w = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    out = dict(tsdf=float(np.abs(got_t[s, l] - tsdf[s, l]).max()), weight_exact=bool((got_w[s, l] == weight[s, l]).all()), stable=int(at.sum()),
               allocated=int(has.sum()))
    if color is not None:
        got_c = vol.color.cpu().numpy()
        out["color"] = float(max(np.abs(got_c[s, c, l] - color[s, c, l]).max() for c in range(3)))
    return out


def test_integrate_parity_after_one_two_and_three_views(views, reference):
    ref, states = reference
    staged = [_stage(vw) for vw in views]
    vol = _volume()
    for st in staged:
        _touch(vol, st)
    assert vol.allocate() == S_BLOCKS == ref.blocks
    assert np.array_equal(vol.block_of_slot.cpu().numpy(), ref.block_of_slot) and np.array_equal(vol.table.cpu().numpy(), ref.table)
    for n, (st, state) in enumerate(zip(staged, states)):
        _integrate(vol, st)
        e = _pool_errors(vol, ref, state)
        print(f"views {n + 1}: tsdf {e['tsdf']:.3e} colour {e['color']:.3e} over {e['stable']} stable of {e['allocated']} allocated nodes")
        assert e["weight_exact"], n
        assert e["stable"] >= 0.99 * e["allocated"]
        assert e["tsdf"] <= INTEGRATE_TOL["tsdf"], (n, e)
        assert e["color"] <= INTEGRATE_TOL["color"], (n, e)
    # to_dense lays the pool out as TSDFVolume's planes, zeros where nothing is allocated
    has, slot, local = _positions(ref.table, ref.blocks, S_DIMS)
    tsdf, weight, color = (t.cpu().numpy() for t in vol.to_dense())
    assert tsdf.shape == S_DIMS[::-1] and color.shape == (3,) + S_DIMS[::-1]
    pool_t, pool_w, pool_c = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy()
    s, l = slot[has], local[has]
    assert np.array_equal(tsdf[has], pool_t[s, l]) and np.array_equal(weight[has], pool_w[s, l])
    assert all(np.array_equal(color[c][has], pool_c[s, c, l]) for c in range(3))
    assert not tsdf[~has].any() and not weight[~has].any() and not color[:, ~has].any()
    assert has.sum() < 0.25 * has.size and (weight[has] > 0).any()


def test_integrate_without_colour_and_alpha(views, reference):
    """The two optional inputs left out: no colour planes, no alpha mask (the corner the mask hides is then touched and fused)."""
    ref, states = _restate(views, color=False, alpha=False)
    staged = [_stage(vw, color=False, alpha=False) for vw in views]
    vol = _two_phase(_volume(color=False), staged)
    assert vol.color is None and vol.blocks == ref.blocks
    assert np.array_equal(vol.block_of_slot.cpu().numpy(), ref.block_of_slot)
    e = _pool_errors(vol, ref, states[-1])
    assert e["weight_exact"] and e["tsdf"] <= INTEGRATE_TOL["tsdf"], e
    assert states[-1][1].sum() > reference[1][-1][1].sum()          # the mask does hide something


def _guarded(shape, pattern, dtype=torch.float32):
    """(buffer, view of `shape` inside it): every byte of the buffer is `pattern`; GUARD elements lie on either side of the view."""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 2 * GUARD, dtype=dtype, device="cuda")
    buf.view(torch.uint8).fill_(pattern)
    return buf, buf[GUARD:GUARD + n].view(shape)


@pytest.mark.parametrize("pattern", [p for p in poison.PATTERNS if p != 0], ids=lambda p: "0x%02X" % p)
def test_only_the_view_s_own_nodes_are_written(views, reference, pattern):
    """Poisoned planes: a skipped node, a node of an edge block that does not exist, the spare slots beyond n_slots and the guard bands all
    keep their bytes."""
    ref, states = reference
    staged = [_stage(vw) for vw in views]
    vol = _volume()
    for st in staged:
        _touch(vol, st)
    assert vol.allocate() == S_BLOCKS
    guards = []
    for name, shape in (("tsdf", (S_BLOCKS + SPARE, 512)), ("weight", (S_BLOCKS + SPARE, 512)), ("color", (S_BLOCKS + SPARE, 3, 512))):
        buf, view = _guarded(shape, pattern)
        setattr(vol, name, view)
        guards.append(buf)
    slots = torch.full((S_BLOCKS + SPARE,), -1, dtype=torch.int32, device="cuda")          # (spare entries: no block; never read)
    slots[:S_BLOCKS] = vol.block_of_slot
    vol.block_of_slot = slots
    assert vol.capacity == S_BLOCKS + SPARE and vol.blocks == S_BLOCKS
    word = np.uint32(pattern * 0x01010101)
    has, slot, local = _positions(ref.table, ref.blocks, S_DIMS)
    keep = np.ones((S_BLOCKS + SPARE, 512), bool)            # pool nodes that must keep their bytes: everything but what a view wrote
    for st, (_, _, _, written, unstable) in zip(staged, states):
        _integrate(vol, st)
        gone = has & (written | unstable)
        keep[slot[gone], local[gone]] = False
        assert keep[:S_BLOCKS].sum() > 20000 and (~keep).sum() > 9000
        for name in ("tsdf", "weight"):
            assert (poison.u32(getattr(vol, name).cpu().numpy())[keep] == word).all(), name
        raw = poison.u32(vol.color.cpu().numpy())
        assert all((raw[:, c][keep] == word).all() for c in range(3))
        if pattern == 0x01:                       # 2.4e-38 as the previous weight: the view's own nodes were written
            own = has & written & ~unstable
            assert (vol.weight.cpu().numpy()[slot[own], local[own]] >= 1).all()
    exists = np.zeros((S_BLOCKS, 512), bool)
    exists[slot[has], local[has]] = True
    assert (~exists).sum() > 0 and keep[:S_BLOCKS][~exists].all()         # (the edge blocks of S are 3, 7 and 1 node thick)
    for buf in guards:
        raw = poison.u32(buf.cpu().numpy())
        assert (raw[:GUARD] == word).all() and (raw[-GUARD:] == word).all()


# ------------------------------------------------------------------------------------------------- extract
def _extract_guarded(vol, nV_expect, nT_expect, min_weight=1.0):
    """gsr_sparse_mesh_count + gsr_sparse_mesh_emit called as SparseTSDFVolume.extract calls them, with ROW_GUARD poisoned rows behind each
    output."""
    from _gsr import check, lib, ptr, stream_ptr
    n = vol.blocks
    scratch = torch.empty(int(lib.gsr_sparse_mesh_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    scratch.fill_(0xA5)
    counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    pool = (ptr(vol.table), ptr(vol.block_of_slot), n, vol.capacity, ptr(vol.tsdf), ptr(vol.weight))
    check(lib.gsr_sparse_mesh_count(*pool, *vol.dims, min_weight, ptr(scratch), scratch.numel(), ptr(counts), stream_ptr("cuda")), "gsr_sparse_mesh_count")
    nV, nT = counts.tolist()
    assert (nV, nT) == (nV_expect, nT_expect)
    verts = torch.full((nV + ROW_GUARD, 3), float("nan"), device="cuda")
    colors = torch.full((nV + ROW_GUARD, 3), float("nan"), device="cuda")
    faces = torch.full((nT + ROW_GUARD, 3), -7, dtype=torch.int32, device="cuda")
    check(lib.gsr_sparse_mesh_emit(*pool, ptr(vol.color), *vol.dims, *vol.origin, vol.voxel_size, min_weight, ptr(scratch), ptr(verts), ptr(colors),
                                   ptr(faces), nV, nT, stream_ptr("cuda")), "gsr_sparse_mesh_emit")
    assert torch.isnan(verts[nV:]).all() and torch.isnan(colors[nV:]).all() and (faces[nT:] == -7).all()
    return verts[:nV], colors[:nV], faces[:nT]


def _ratio(got, want, bound):
    return float((np.abs(got.astype(np.float64) - want) / bound).max()) if len(want) else 0.0


def _assert_extraction(vol, restated, name):
    """The raw entries behind guard rows against sparse_ref.extract's (V, C, F, ..., ends), then SparseTSDFVolume.extract."""
    V, C, F, _, _, ends = restated
    verts, colors, faces = _extract_guarded(vol, len(V), len(F))
    assert (faces.cpu().numpy() == F).all()
    pos, col = M.extract_bounds(ends, vol.voxel_size)
    rv, rc = _ratio(verts.cpu().numpy(), V, pos), _ratio(colors.cpu().numpy(), C, col)
    print(f"{name}: {vol.blocks} slots, nV {len(V)} nT {len(F)}, |device - restatement| / bound: positions {rv:.3f} colours {rc:.3f}")
    assert rv <= 1.0 and rc <= 1.0
    for _ in range(2):                                         # the Python layer gives the same bytes, twice
        mesh = vol.extract()
        assert torch.equal(mesh.vertices, verts) and torch.equal(mesh.faces, faces) and torch.equal(mesh.colors, colors)
    assert mesh.faces.dtype == torch.int32 and mesh.vertices.is_cuda
    return len(V), len(F)


def _restate_device_pool(vol):
    """sparse_ref.extract evaluated on the device's own table and planes."""
    return R.extract(vol.table.cpu().numpy(), vol.block_of_slot.cpu().numpy(), vol.blocks, vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(),
                     None if vol.color is None else vol.color.cpu().numpy(), vol.dims, vol.origin, vol.voxel_size)


def test_extraction_of_the_fused_fixture(views):
    vol = _two_phase(_volume(), [_stage(vw) for vw in views])
    nV, nT = _assert_extraction(vol, _restate_device_pool(vol), "S")
    assert abs(nV - 4709) <= 47 and abs(nT - 8670) <= 87          # the float64 fusion gives 4709 and 8670 (tests/test_sparse_ref.py)
    bare = _two_phase(_volume(color=False), [_stage(vw, color=False) for vw in views])
    mesh, with_colour = bare.extract(), vol.extract()
    assert mesh.colors is None and torch.equal(mesh.vertices, with_colour.vertices) and torch.equal(mesh.faces, with_colour.faces)


def _from_dense(grid, dims, slot_blocks, origin=M.GRID_ORIGIN, voxel=M.GRID_VOXEL):
    """A SparseTSDFVolume whose slots 0, 1, ... hold the blocks `slot_blocks` of the dense grid (tsdf, weight, color).  The pool nodes that
    do not exist hold tsdf -1 and weight 5: inside and valid, were they ever read."""
    tsdf, weight, color = grid
    n = len(slot_blocks)
    table = np.full(int(np.prod(R.grid(dims))), R.UNTOUCHED, np.int32)
    table[slot_blocks] = np.arange(n)
    has, slot, local = _positions(table, n, dims)
    pool_t, pool_w, pool_c = np.full((n, 512), -1.0, np.float32), np.full((n, 512), 5.0, np.float32), np.full((n, 3, 512), 0.25, np.float32)
    s, l = slot[has], local[has]
    pool_t[s, l], pool_w[s, l] = tsdf[has], weight[has]
    for c in range(3):
        pool_c[s, c, l] = color[c][has]
    vol = _volume(dims, origin, voxel)
    vol.table, vol.block_of_slot = _dev(table, torch.int32), _dev(np.asarray(slot_blocks), torch.int32)
    vol.tsdf, vol.weight, vol.color = _dev(pool_t), _dev(pool_w), _dev(pool_c)
    vol._blocks = n
    vol.counts.fill_(n)
    return vol, has


def test_random_lattice_with_a_random_subset_of_its_blocks_in_shuffled_slots():
    """20 x 17 x 19 nodes in 3 x 3 x 3 blocks (the last 4, 1 and 3 nodes thick), 17 of them allocated: cells and edges that cross into a
    block without storage, exact zeros, scattered invalid nodes."""
    dims = (20, 17, 19)
    grid = M.random_lattice(dims, 21, 0.08, True)
    slot_blocks = np.random.RandomState(3).permutation(27)[:17]
    vol, has = _from_dense(grid, dims, slot_blocks)
    assert 0.4 < has.mean() < 0.9 and (grid[0][has] == 0).sum() > 20 and np.isnan(grid[1][has]).sum() > 5
    nV, nT = _assert_extraction(vol, _restate_device_pool(vol), "20x17x19 subset")
    assert nT > 2000
    # the dense planes with the other blocks invalid give the same mesh, permuted
    tsdf, weight, color = grid
    masked = (tsdf, np.where(has, weight, 0).astype(np.float32), color)
    V, C, F, keys, face_cells, _ = _restate_device_pool(vol)
    Vp, Cp, Fp = R.to_pool_order(M.extract(*masked, M.GRID_ORIGIN, M.GRID_VOXEL), R.dense_keys(masked[0], masked[1]), keys, face_cells)
    assert np.array_equal(V, Vp) and np.array_equal(C, Cp) and np.array_equal(F, Fp)


@pytest.mark.parametrize("dims", [(2, 2, 2), (8, 8, 8), (9, 8, 8), (20, 17, 19)], ids=lambda d: "x".join(map(str, d)))
def test_all_blocks_allocated_against_the_dense_restatement(dims):
    """Every block has a slot (in shuffled order): the mesh is mesh_ref.extract's of the same planes, in pool order.  2 x 2 x 2 is one cell
    in one block; 8 x 8 x 8 one full block; 9 x 8 x 8 adds a block one node thick."""
    p_invalid = 0.0 if dims == (2, 2, 2) else 0.05
    grid = M.random_lattice(dims, 30 + sum(dims), p_invalid, dims != (2, 2, 2))
    if dims == (2, 2, 2):
        grid[0][0, 0, 0], grid[0][1, 1, 1] = -0.5, 0.25              # one sign change at least
    G = int(np.prod(R.grid(dims)))
    vol, has = _from_dense(grid, dims, np.random.RandomState(G).permutation(G))
    assert has.all()
    restated = _restate_device_pool(vol)
    nV, nT = _assert_extraction(vol, restated, "x".join(map(str, dims)))
    assert nT > 0
    V, C, F, keys, face_cells, _ = restated
    Vp, Cp, Fp = R.to_pool_order(M.extract(*grid, M.GRID_ORIGIN, M.GRID_VOXEL), R.dense_keys(grid[0], grid[1]), keys, face_cells)
    assert np.array_equal(V, Vp) and np.array_equal(C, Cp) and np.array_equal(F, Fp)


def test_a_pool_longer_than_one_round_of_the_spine():
    """2 x 2 x 4165 nodes, 521 blocks, all allocated in shuffled order: 1042 scan blocks of 256 pool nodes, so the bases of the last 18
    come from the 64-bit carries of scan_spine_kernel's second round."""
    dims = (2, 2, 8 * 520 + 5)
    grid = M.random_lattice(dims, 23, 0.05, True)
    vol, has = _from_dense(grid, dims, np.random.RandomState(5).permutation(521), origin=M.COLUMN_ORIGIN, voxel=0.001)
    assert has.all() and vol.blocks * 2 > 1024 + 16
    restated = _restate_device_pool(vol)
    nV, nT = _assert_extraction(vol, restated, "thin column")
    assert nV > 5000 and nT > 5000


def test_empty_surfaces_give_empty_tensors(views):
    fresh = _volume()
    for vol in (fresh, _volume(color=False)):
        mesh = vol.extract()
        assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and mesh.faces.dtype == torch.int32
        assert (mesh.colors is None) == (vol.color is None) and (mesh.colors is None or mesh.colors.shape == (0, 3))
    staged = [_stage(vw) for vw in views]
    for st in staged:
        _touch(fresh, st)
    assert fresh.allocate() == S_BLOCKS
    assert fresh.extract().faces.shape == (0, 3)                   # allocated, nothing fused: every node invalid
    _integrate(fresh, staged[0])
    assert fresh.extract(min_weight=2.0).vertices.shape == (0, 3) and fresh.extract().vertices.shape[0] > 0
    fresh.integrate(staged[0][0], staged[0][1], rgb=staged[0][2], alpha=staged[0][3], **FIX)
    assert fresh.extract(min_weight=2.0).vertices.shape[0] > 0


# ------------------------------------------------------------------------------------------------- against the dense device path
def test_every_emitting_cell_of_the_dense_volume_is_allocated(views, reference):
    """TSDFVolume and SparseTSDFVolume over S, the same three views: each cell that emits in the dense volume has its eight nodes allocated
    (in the float64 restatement all of them do, tests/test_sparse_ref.py); a cell within two nodes of an unstable node is excused, at most
    1 % of the emitting cells.  The allocated nodes hold the dense volume's values."""
    import gsr_mesh
    staged = [_stage(vw) for vw in views]
    sparse = _two_phase(_volume(), staged)
    dense = gsr_mesh.TSDFVolume(M.FIX_ORIGIN, S_VOXEL, S_DIMS, "cuda", color=True)
    for st in staged:
        _integrate(dense, st)
    tsdf, weight = dense.tsdf.cpu().numpy(), dense.weight.cpu().numpy()
    nz, ny, nx = tsdf.shape
    corners = lambda a: [a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    valid, inside = weight >= 1, tsdf < 0
    emits = np.all(corners(valid), 0) & np.any(corners(inside), 0) & ~np.all(corners(inside), 0)
    has, slot, local = _positions(sparse.table.cpu().numpy(), sparse.blocks, S_DIMS)
    complete = np.all(corners(has), 0)
    unstable = reference[1][-1][4]
    near = np.zeros((nz + 4, ny + 4, nx + 4), bool)
    for dz in range(5):
        for dy in range(5):
            for dx in range(5):
                near[dz:dz + nz, dy:dy + ny, dx:dx + nx] |= unstable
    excused = emits & ~complete & np.any(corners(near[2:-2, 2:-2, 2:-2]), 0)
    print(f"dense path: {int(emits.sum())} emitting cells, {int((emits & ~complete).sum())} incomplete, {int(excused.sum())} excused")
    assert emits.sum() > 1000
    assert not (emits & ~complete & ~excused).any()
    assert excused.sum() <= 0.01 * emits.sum()
    # the same updates in the same order: the allocated nodes hold what the dense kernel gave (both within INTEGRATE_TOL of float64)
    st, sw, sc = (t.cpu().numpy() for t in sparse.to_dense())
    assert np.array_equal(sw[has], weight[has])
    assert np.abs(st[has] - tsdf[has]).max() <= 2 * INTEGRATE_TOL["tsdf"]
    assert np.abs(sc[:, has] - dense.color.cpu().numpy()[:, has]).max() <= 2 * INTEGRATE_TOL["color"]
    if not (emits & ~complete).any():
        a, b = sparse.extract(), dense.extract()
        assert a.vertices.shape == b.vertices.shape and a.faces.shape == b.faces.shape


# ------------------------------------------------------------------------------------------------- streams
def test_the_four_steps_on_a_side_stream_behind_a_producer(views):
    """The depth map is produced on the side stream right in front of touch and integrate, allocate and extract follow, and the host waits
    only where they read their counts: equal to the default-stream result."""
    def run(stream):
        vol = _volume()
        inputs = [_stage(vw) for vw in views]
        big = torch.randn(4_000_000, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())            # the fills and the uploads above ran on the default stream
        with torch.cuda.stream(stream):
            produced = []
            for staged, cam, rgb, alpha in inputs:
                for _ in range(4):
                    big = big * 1.0001 + 0.5                       # keeps the stream busy in front of the producer
                depth = staged * 0.5
                depth.mul_(2.0)                                    # the producer (exact: a power of two)
                _touch(vol, (depth, cam, rgb, alpha))
                produced.append((depth, cam, rgb, alpha))
            vol.allocate()
            for st in produced:
                big = big * 1.0001 + 0.5
                _integrate(vol, st)
            mesh = vol.extract()
        stream.synchronize()
        return vol, mesh
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    vol_s, mesh_s = run(side)
    vol_d, mesh_d = run(torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert vol_s.blocks == vol_d.blocks == S_BLOCKS
    for name in ("table", "block_of_slot", "tsdf", "weight", "color"):
        assert torch.equal(getattr(vol_s, name), getattr(vol_d, name)), name
    assert mesh_s.vertices.shape[0] > 0
    for a, b in zip(mesh_s, mesh_d):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- end to end
BALL_RADIUS = 2.0


def _ball_model(P=4000, seed=1000, L=16):
    import gsr_synth as S
    from cubemapencoder import CubemapEncoder
    sc = S.make_scene(P, ball=True, seed=seed)
    tex, fail = S.make_cubemap(L, 3, seed)
    t = {k: torch.from_numpy(sc[k]).cuda() for k in ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")}
    env = CubemapEncoder(output_dim=3, resolution=L).cuda()
    with torch.no_grad():
        env.params["Cubemap_texture"].copy_(torch.from_numpy(tex))
        env.params["Cubemap_failv"].copy_(torch.from_numpy(fail))

    class PC:
        get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (t["means3D"], t["opacities"], t["scales"], t["rotations"],
                                                                                   t["shs"], t["refl_strengths"])
        active_sh_degree, get_envmap = 3, env

    class Pipe:
        depth_ratio, compute_cov3D_python = 0.0, False
    return PC, Pipe


@pytest.fixture(scope="module")
def extractor():
    import gsr_synth as S
    from gaussian_renderer import render
    from utils.mesh_utils import GaussianExtractor
    PC, Pipe = _ball_model()
    cams = S.circle_cameras(96, 64, n=6)
    ex = GaussianExtractor(PC, render, Pipe)
    ex.reconstruction([cameras.view_of(c) for c in cams])
    return ex, cams


def test_extract_mesh_bounded_sparse_gives_the_dense_call_s_mesh(extractor):
    ex, cams = extractor
    args = dict(voxel_size=0.05, sdf_trunc=0.2, depth_trunc=10)
    sparse, dense = ex.extract_mesh_bounded(sparse=True, **args), ex.extract_mesh_bounded(**args)
    assert sparse.vertices.shape[0] > 1000 and sparse.faces.shape[0] > 1000
    assert sparse.vertices.shape == dense.vertices.shape and sparse.faces.shape == dense.faces.shape and sparse.colors.shape == dense.colors.shape
    assert int(sparse.faces.max()) == sparse.vertices.shape[0] - 1 and int(sparse.faces.min()) == 0
    t = M.topology(sparse.faces.cpu().numpy(), sparse.vertices.shape[0])
    assert t["unreferenced"] == 0 and t["nonmanifold"] == 0 and t["repeated_directed"] == 0
    # the restatement on the downloaded maps, over the volume extract_mesh_bounded lays out (as tests/test_gpu_mesh.py's end to end)
    centre, radius = ex.camera_bounds()
    lo = [float(c) - radius for c in centre]
    dims = tuple(max(2, int(np.ceil(2 * radius / 0.05)) + 1) for _ in range(3))
    ref = M.Volume(dims, lo, 0.05, color=False)
    for cam, depth, alpha in zip(cams, ex.depthmaps, ex.alphamaps):
        M.integrate(ref, depth[0].cpu().numpy(), None, alpha[0].cpu().numpy(), 0.5, cam["viewmatrix"], cam["projmatrix"], 0.2, 10.0)
    vr = M.extract_vertices(ref.tsdf.astype(np.float32), ref.weight.astype(np.float32), ref.origin.astype(np.float64), ref.voxel)
    stat = lambda p: float(np.median(np.abs(np.linalg.norm(p, axis=1) - BALL_RADIUS)))
    device, restated = stat(sparse.vertices.cpu().numpy().astype(np.float64)), stat(vr)
    print(f"end to end: {sparse.vertices.shape[0]} vertices ({len(vr)} in the restatement), median | |v| - R |: device {device:.4f}, restatement {restated:.4f}")
    assert abs(sparse.vertices.shape[0] - len(vr)) <= 0.01 * len(vr)
    assert device <= 2 * restated


def test_extract_mesh_bounded_sparse_where_the_dense_volume_cannot_exist(extractor):
    """A column of 1 x 1 through the ball, 138 long, at voxel 0.004: 251 x 251 x 34501 = 2.17e9 nodes, which the dense path refuses; the
    band of the six views stays a small share of the 4.4 million blocks.  The mesh is held to what the dense end-to-end test holds its mesh
    to (every index in range, no unreferenced vertex, no non-manifold or repeated directed edge).  It is NOT closed in the sense of having
    no boundary edge, and no bounded extraction of this model is, dense or sparse: observed on an MI355X, 1 255 826 vertices, 2 382 544
    faces, 127 156 boundary edges of 3 637 394 — the column's faces cut the surface, and six cameras in a ring see neither the poles of
    the ball nor anything behind the first surfels."""
    import gsr_mesh
    ex, _ = extractor
    args = dict(voxel_size=0.004, sdf_trunc=0.02, depth_trunc=10, bounds=((-0.5, -0.5, -69.0), (0.5, 0.5, 69.0)))
    with pytest.raises(ValueError, match=r"251 x 251 x 34501 = \d+ nodes.*sparse=True"):
        ex.extract_mesh_bounded(**args)
    assert 251 * 251 * 34501 > gsr_mesh.MAX_NODES
    mesh = ex.extract_mesh_bounded(sparse=True, **args)
    nV, nT = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    t = M.topology(mesh.faces.cpu().numpy(), nV)
    print(f"column: {nV} vertices, {nT} faces, {t['boundary']} boundary edges of {t['E']}")
    assert nV > 1000 and nT > 1000 and mesh.colors.shape == (nV, 3)
    assert int(mesh.faces.max()) == nV - 1 and int(mesh.faces.min()) == 0
    assert t["unreferenced"] == 0 and t["nonmanifold"] == 0 and t["repeated_directed"] == 0
    v = mesh.vertices.cpu().numpy()
    assert (np.abs(v[:, :2]) <= 0.5 + 1e-3).all() and np.abs(v[:, 2]).max() < 6.0          # inside the column, within the cameras' ring
    with pytest.raises(ValueError, match="2\\^31 - 1 of a sparse volume"):
        ex.extract_mesh_bounded(sparse=True, voxel_size=0.004, bounds=((-70, -70, -70), (70, 70, 70)))
