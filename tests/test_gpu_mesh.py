"""gsr_mesh on the GPU against the float64 restatement (tests/mesh_ref.py): TSDF integration over one, two and three views, the rule that a
skipped node is not written, the marching-tetrahedra extraction (counts and faces exactly, positions within a recorded tolerance), stream
ordering, and GaussianExtractor end to end.  The extraction is held face by face on three analytic grids and on lattices without
structure (random signs, exact zeros, scattered invalid nodes, every corner configuration, dimensions of 2, more than 1024 blocks).

Tolerances.  The restatement is float64 on the float32 inputs, so what is compared is the device's float32 rounding.  Each tolerance is
four times the largest error observed on an MI355X against the restatement (gpu_mesh_figures() prints the figures; DESIGN.md, "Mesh
extraction" records them): four times lets a change of instruction order move a few ulps through the divisions, while a wrong pixel
convention or a transposed matrix is off by orders of magnitude.  The lattice tests do not use an observed figure: their bound per vertex
follows from the emit kernel's arithmetic (mesh_ref.extract_bounds).
"""
import numpy as np
import pytest
import torch

import cameras
import mesh_ref as M
import poison

pytestmark = pytest.mark.gpu

# largest |device - restatement| observed on an MI355X, and the tolerances that follow
INTEGRATE_OBSERVED = {"tsdf": 3.18e-7, "color": 5.97e-8}      # over the fixture's three views, the run without colour and alpha, the thin column
EXTRACT_OBSERVED = {"verts": 2.46e-7, "colors": 7.64e-8}       # over the three grids (vertex coordinates up to 4.6)
INTEGRATE_TOL = {k: 4 * v for k, v in INTEGRATE_OBSERVED.items()}
EXTRACT_TOL = {k: 4 * v for k, v in EXTRACT_OBSERVED.items()}
# end to end: median | |v| - R | as observed, device and float64 restatement on the downloaded depth maps (185392 and 185390 vertices: 4000
# random surfels are no surface, and a few pixels carry depths up to 80); the test allows the device twice the restatement's figure of its run
E2E_OBSERVED = {"reference": 0.58308, "device": 0.58309}
GUARD = 64                       # floats in front of and behind each guarded plane


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _guarded(shape, pattern, dtype=torch.float32):
    """(buffer, view of `shape` inside it): every byte of the buffer is `pattern`; GUARD elements lie on either side of the view."""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 2 * GUARD, dtype=dtype, device="cuda")
    buf.view(torch.uint8).fill_(pattern)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _volume(dims=M.FIX_DIMS, origin=M.FIX_ORIGIN, voxel=M.FIX_VOXEL, color=True, pattern=None):
    """A TSDFVolume; with `pattern`, its planes are views into guarded buffers filled with it (returned as .guards)."""
    import gsr_mesh
    vol = gsr_mesh.TSDFVolume(origin, voxel, dims, "cuda", color=color)
    vol.guards = []
    if pattern is not None:
        for name in ("tsdf", "weight") + (("color",) if color else ()):
            buf, view = _guarded(tuple(getattr(vol, name).shape), pattern)
            setattr(vol, name, view)
            vol.guards.append(buf)
    return vol


def _stage(vw, color=True, alpha=True):
    """The view's inputs on the device: (depth, camera object, rgb | None, alpha | None)."""
    return (_dev(vw["depth"]), cameras.view_of(vw["cam"]), _dev(vw["rgb"]) if color else None, _dev(vw["alpha"]) if alpha else None)


def _integrate(vol, vw, color=True, alpha=True, staged=None):
    depth, cam, rgb, a = _stage(vw, color, alpha) if staged is None else staged
    vol.integrate(depth, cam, rgb=rgb, alpha=a, alpha_min=M.FIX_ALPHA_MIN, sdf_trunc=M.FIX_SDF_TRUNC, depth_trunc=M.FIX_DEPTH_TRUNC)


@pytest.fixture(scope="module")
def views():
    return M.integrate_fixture()


@pytest.fixture(scope="module")
def reference(views):
    return M.integrate_reference(views)


def integrate_errors(views, reference):
    """Per number of views: largest |device - restatement| of tsdf and colour over the stable nodes, and whether weight is exact there."""
    vol = _volume()
    out = []
    for vw, (tsdf, weight, color, _, unstable) in zip(views, reference):
        _integrate(vol, vw)
        ok = ~unstable
        out.append(dict(tsdf=float(np.abs(vol.tsdf.cpu().numpy() - tsdf)[ok].max()), color=float(np.abs(vol.color.cpu().numpy() - color)[:, ok].max()),
                        weight_exact=bool((vol.weight.cpu().numpy() == weight)[ok].all()), stable=int(ok.sum())))
    return out


def test_integrate_parity_after_one_two_and_three_views(views, reference):
    for n, e in enumerate(integrate_errors(views, reference)):
        print(f"views {n + 1}: tsdf {e['tsdf']:.3e} colour {e['color']:.3e} over {e['stable']} stable nodes")
        assert e["weight_exact"], n
        assert e["stable"] >= 0.99 * np.prod(M.FIX_DIMS)
        assert e["tsdf"] <= INTEGRATE_TOL["tsdf"], (n, e)
        assert e["color"] <= INTEGRATE_TOL["color"], (n, e)


def test_integrate_without_colour_and_alpha(views):
    """The entry's two optional inputs left out: no colour planes, no alpha mask (the corner the mask hides is then fused)."""
    vol, ref = _volume(color=False), M.Volume(M.FIX_DIMS, M.FIX_ORIGIN, M.FIX_VOXEL, color=False)
    unstable = np.zeros(ref.tsdf.shape, bool)
    masked = M.integrate_reference(views, color=False)
    for vw in views:
        _integrate(vol, vw, color=False, alpha=False)
        _, uns = M.integrate(ref, vw["depth"], None, None, M.FIX_ALPHA_MIN, vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"], M.FIX_SDF_TRUNC,
                             M.FIX_DEPTH_TRUNC)
        unstable |= uns
    ok = ~unstable
    assert (vol.weight.cpu().numpy() == ref.weight)[ok].all()
    assert np.abs(vol.tsdf.cpu().numpy() - ref.tsdf)[ok].max() <= INTEGRATE_TOL["tsdf"]
    assert ref.weight.sum() > masked[-1][1].sum()          # the mask does hide something


@pytest.mark.parametrize("pattern", [p for p in poison.PATTERNS if p != 0], ids=lambda p: "0x%02X" % p)
def test_a_skipped_node_is_not_written_and_the_guard_bands_stay(views, reference, pattern):
    vol = _volume(pattern=pattern)
    word = np.uint32(pattern * 0x01010101)
    written_any = np.zeros(M.FIX_DIMS[::-1], bool)
    for vw, (_, _, _, written, unstable) in zip(views, reference):
        _integrate(vol, vw)
        written_any |= written
        keep = ~written_any & ~unstable
        assert keep.sum() > 0.5 * keep.size
        for name in ("tsdf", "weight"):
            assert (poison.u32(getattr(vol, name).cpu().numpy())[keep] == word).all(), name
        assert (poison.u32(vol.color.cpu().numpy())[:, keep] == word).all()
        touched = written & ~unstable
        if pattern == 0x01:                     # 2.4e-38 as the previous weight: the view's own nodes were written
            assert (vol.weight.cpu().numpy()[touched] >= 1).all()
    for buf in vol.guards:
        raw = poison.u32(buf.cpu().numpy())
        assert (raw[:GUARD] == word).all() and (raw[-GUARD:] == word).all()


def test_thin_column_volume_walks_the_grid_in_strides():
    """2 x 2 x 560001 nodes: ragged against the block in every axis, and 70001 blocks where a launch holds 65536, so the kernel's stride
    over the blocks is taken."""
    dims, origin, voxel = (2, 2, 560001), (-0.2, 0.1, 0.3), 5e-6
    cam = cameras.family("offcentre", M.FIX_W, M.FIX_H, 20)
    depth = M.ray_depth_map(cam, (-0.2, 0.1, 1.6), 0.4, np.array([0.0, 0.0, 1.0]), 2.4)
    vw = dict(cam=cam, depth=depth, rgb=None, alpha=None)
    vol, ref = _volume(dims, origin, voxel, color=False), M.Volume(dims, origin, voxel, color=False)
    _integrate(vol, vw, color=False, alpha=False)
    written, unstable = M.integrate(ref, depth, None, None, 0.5, cam["viewmatrix"], cam["projmatrix"], M.FIX_SDF_TRUNC, M.FIX_DEPTH_TRUNC)
    ok = ~unstable
    assert unstable.mean() <= 0.01 and 0.2 < written.mean() < 0.8
    assert (vol.weight.cpu().numpy() == ref.weight)[ok].all()
    assert np.abs(vol.tsdf.cpu().numpy() - ref.tsdf)[ok].max() <= INTEGRATE_TOL["tsdf"]


# ------------------------------------------------------------------------------------------------- extraction
GRIDS = {"sphere": lambda: M.sphere_grid(), "torus": lambda: M.torus_grid(), "cut-sphere": lambda: M.sphere_grid(cut_x=9)}
ROW_GUARD = 16                   # rows behind verts, colours and faces


@pytest.fixture(scope="module")
def extracted():
    return {name: (make(), M.extract(*make(), M.GRID_ORIGIN, M.GRID_VOXEL)) for name, make in GRIDS.items()}


def _upload(grid, dims=M.GRID, origin=M.GRID_ORIGIN, voxel=M.GRID_VOXEL):
    tsdf, weight, color = grid
    vol = _volume(dims, origin, voxel, color=color is not None)
    vol.tsdf.copy_(_dev(tsdf))
    vol.weight.copy_(_dev(weight))
    if color is not None:
        vol.color.copy_(_dev(color))
    return vol


def _extract_guarded(vol, nV_expect, nT_expect, min_weight=1.0):
    """gsr_mesh_count + gsr_mesh_emit called as TSDFVolume.extract calls them, with ROW_GUARD poisoned rows behind each output."""
    from _gsr import check, lib, ptr, stream_ptr
    nx, ny, nz = vol.dims
    scratch = torch.empty(int(lib.gsr_mesh_scratch_bytes(nx, ny, nz)), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    check(lib.gsr_mesh_count(ptr(vol.tsdf), ptr(vol.weight), nx, ny, nz, min_weight, ptr(scratch), scratch.numel(), ptr(counts), stream_ptr("cuda")),
          "gsr_mesh_count")
    nV, nT = counts.tolist()
    assert (nV, nT) == (nV_expect, nT_expect)
    verts = torch.full((nV + ROW_GUARD, 3), float("nan"), device="cuda")
    colors = torch.full((nV + ROW_GUARD, 3), float("nan"), device="cuda")
    faces = torch.full((nT + ROW_GUARD, 3), -7, dtype=torch.int32, device="cuda")
    check(lib.gsr_mesh_emit(ptr(vol.tsdf), ptr(vol.weight), ptr(vol.color), nx, ny, nz, *vol.origin, vol.voxel_size, min_weight, ptr(scratch), ptr(verts),
                            ptr(colors), ptr(faces), nV, nT, stream_ptr("cuda")), "gsr_mesh_emit")
    assert torch.isnan(verts[nV:]).all() and torch.isnan(colors[nV:]).all() and (faces[nT:] == -7).all()
    return verts[:nV], colors[:nV], faces[:nT]


def extract_errors(extracted):
    out = {}
    for name, (grid, (V, C, F)) in extracted.items():
        mesh = _upload(grid).extract()
        same = tuple(mesh.faces.shape) == F.shape and bool((mesh.faces.cpu().numpy() == F).all())
        out[name] = dict(nV=int(mesh.vertices.shape[0]), nT=int(mesh.faces.shape[0]), faces_equal=same,
                         verts=float(np.abs(mesh.vertices.cpu().numpy() - V).max()) if same else float("inf"),
                         colors=float(np.abs(mesh.colors.cpu().numpy() - C).max()) if same else float("inf"))
    return out


@pytest.mark.parametrize("name", list(GRIDS))
def test_extraction_parity(extracted, name):
    grid, (V, C, F) = extracted[name]
    vol = _upload(grid)
    verts, colors, faces = _extract_guarded(vol, len(V), len(F))
    assert (faces.cpu().numpy() == F).all()
    ev, ec = float(np.abs(verts.cpu().numpy() - V).max()), float(np.abs(colors.cpu().numpy() - C).max())
    print(f"{name}: nV {len(V)} nT {len(F)} verts {ev:.3e} colours {ec:.3e}")
    assert ev <= EXTRACT_TOL["verts"] and ec <= EXTRACT_TOL["colors"]
    # the Python layer gives the same bytes, twice
    for _ in range(2):
        mesh = vol.extract()
        assert torch.equal(mesh.vertices, verts) and torch.equal(mesh.faces, faces) and torch.equal(mesh.colors, colors)
    assert mesh.faces.dtype == torch.int32 and mesh.vertices.is_cuda
    # without colour: the same geometry, no colour tensor
    bare = _upload((grid[0], grid[1], None)).extract()
    assert bare.colors is None and torch.equal(bare.vertices, verts) and torch.equal(bare.faces, faces)


def test_min_weight_decides_validity(extracted):
    """weight 1 everywhere: min_weight = 2 makes every node invalid, min_weight = 0 also takes the unobserved column in."""
    grid, (V, C, F) = extracted["cut-sphere"]
    vol = _upload(grid)
    empty = vol.extract(min_weight=2.0)
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
    Va, _, Fa = M.extract(*grid, M.GRID_ORIGIN, M.GRID_VOXEL, min_weight=0.0)
    all_in = vol.extract(min_weight=0.0)
    assert (all_in.faces.cpu().numpy() == Fa).all() and np.abs(all_in.vertices.cpu().numpy() - Va).max() <= EXTRACT_TOL["verts"]
    assert len(Fa) != len(F)


def test_empty_surfaces_give_empty_tensors(extracted):
    (tsdf, weight, color), _ = extracted["sphere"]
    for t, w in ((np.abs(tsdf) + 1, weight), (tsdf, np.zeros_like(weight))):
        mesh = _upload((t, w, color)).extract()
        assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and mesh.colors.shape == (0, 3)
        assert mesh.faces.dtype == torch.int32
    vol = _upload((tsdf, weight, color))
    vol.reset()
    assert float(vol.tsdf.abs().sum() + vol.weight.abs().sum() + vol.color.abs().sum()) == 0.0
    assert vol.extract().faces.shape == (0, 3)


# ------------------------------------------------------------------------------------------------- extraction on lattices without structure
# Counts and every face index exactly.  Positions and colours within mesh_ref.extract_bounds(): a bound per vertex and component that
# follows from the kernel's arithmetic (four roundings of max(|a|, |b|) and four of the voxel; four of max(|ca|, |cb|)), not from what the
# kernel gave.  LATTICE_OBSERVED records the largest |device - restatement| / bound seen on an MI355X (each test prints its own).
LATTICE_OBSERVED = {"verts": 0.481, "colors": 0.516}              # the long column; the lattice at min_weight 0
SMALL_DIMS = ((2, 2, 2), (3, 2, 2), (2, 3, 2), (2, 2, 3), (65, 2, 3), (2, 257, 2))
GRID_LATTICES = ((1, 0.0), (2, 0.0), (3, 0.08), (4, 0.08))          # (seed, p_invalid) on mesh_ref.GRID
MIN_WEIGHTS = (0.0, 0.5, 2.0)                                       # each a value the lattice's weights take


def _lattice_cases():
    """{name: (grid, dims, origin, voxel[, min_weight])}."""
    cases = {}
    for seed, p in GRID_LATTICES:
        cases[f"grid-p{p}-seed{seed}"] = (M.random_lattice(M.GRID, seed, p, True), M.GRID, M.GRID_ORIGIN, M.GRID_VOXEL)
    for w in MIN_WEIGHTS:
        tsdf, weight, color = M.random_lattice(M.GRID, 5, 0.3, True)
        cases[f"min-weight-{w}"] = ((tsdf, weight * (2 if w == 2.0 else 1), color), M.GRID, M.GRID_ORIGIN, M.GRID_VOXEL, w)
    cases["configs"] = (M.config_lattice(), M.CONFIG_DIMS, (-0.4, 0.2, -1.3), 0.01)
    for n, dims in enumerate(SMALL_DIMS):
        cases["x".join(map(str, dims))] = (M.random_lattice(dims, 10 + n, 0.05 if max(dims) > 3 else 0.0, True), dims, M.GRID_ORIGIN, M.GRID_VOXEL)
    tsdf, weight, color = M.random_lattice((2, 2, 2), 10, 0.0, False)
    cases["2x2x2-all-inside"] = ((-np.abs(tsdf), weight, color), (2, 2, 2), M.GRID_ORIGIN, M.GRID_VOXEL)
    for name, bad in (("zero", 0.0), ("nan", np.nan), ("half", 0.5)):
        w = weight.copy()
        w[1, 0, 1] = bad
        cases[f"2x2x2-one-corner-{name}"] = ((tsdf, w, color), (2, 2, 2), M.GRID_ORIGIN, M.GRID_VOXEL)
    return cases


@pytest.fixture(scope="module")
def lattices():
    """{name: (grid, dims, origin, voxel, min_weight, (V, C, F, ends))}, each restated once."""
    out = {}
    for name, case in _lattice_cases().items():
        grid, dims, origin, voxel, min_weight = case if len(case) == 5 else case + (1.0,)
        out[name] = (grid, dims, origin, voxel, min_weight, M.extract(*grid, origin, voxel, min_weight, ends=True))
    blocks, order, gap = M.long_column()
    tsdf, weight, color, k0 = M.stacked(blocks, order, gap)
    out["column"] = ((tsdf, weight, color), tsdf.shape[::-1], M.COLUMN_ORIGIN, M.COLUMN_VOXEL, 1.0,
                     M.stacked_mesh(blocks, order, k0, M.COLUMN_ORIGIN, M.COLUMN_VOXEL))
    return out


def _ratio(got, want, bound):
    return float((np.abs(got.astype(np.float64) - want) / bound).max()) if len(want) else 0.0


def _assert_extraction(case, name):
    """The raw entries behind guard rows, then TSDFVolume.extract with and without colour; returns (nV, nT, position ratio, colour ratio)."""
    grid, dims, origin, voxel, min_weight, (V, C, F, ends) = case
    vol = _upload(grid, dims, origin, voxel)
    verts, colors, faces = _extract_guarded(vol, len(V), len(F), min_weight)
    assert (faces.cpu().numpy() == F).all()
    pos, col = M.extract_bounds(ends, voxel)
    rv, rc = _ratio(verts.cpu().numpy(), V, pos), _ratio(colors.cpu().numpy(), C, col)
    print(f"{name}: {int(np.prod(dims))} nodes, nV {len(V)} nT {len(F)}, |device - restatement| / bound: positions {rv:.3f} colours {rc:.3f}")
    assert rv <= 1.0 and rc <= 1.0
    mesh = vol.extract(min_weight)
    assert torch.equal(mesh.vertices, verts) and torch.equal(mesh.faces, faces) and torch.equal(mesh.colors, colors)
    bare = _upload((grid[0], grid[1], None), dims, origin, voxel).extract(min_weight)
    assert bare.colors is None and torch.equal(bare.vertices, verts) and torch.equal(bare.faces, faces)
    return len(V), len(F), rv, rc


@pytest.mark.parametrize("name", [f"grid-p{p}-seed{seed}" for seed, p in GRID_LATTICES])
def test_random_lattices_face_by_face(lattices, name):
    """No structure: every case of the table, exact zeros of both signs, and (p = 0.08) invalid nodes scattered so that an edge is held by
    none, some or all of its cells, with weights at min_weight, below it and NaN (tests/test_mesh_ref.py holds the inputs to that)."""
    nV, nT, _, _ = _assert_extraction(lattices[name], name)
    assert nT > 5000
    tsdf, weight, _ = lattices[name][0]
    assert (tsdf == 0).sum() > 50 and ("p0.0-" in name or np.isnan(weight).sum() > 20)


@pytest.mark.parametrize("min_weight", MIN_WEIGHTS)
def test_a_weight_equal_to_min_weight_is_valid_on_a_lattice(lattices, min_weight):
    """Weights drawn from {0, 0.5, 1, 2, NaN}, three in ten of them from {0, 0.5, NaN}: at min_weight 0 only NaN is invalid, at 0.5 the
    nodes at 0.5 come in; with every weight doubled, min_weight 2 keeps {2, 4} and drops {0, 1, NaN}.  Each threshold is a weight the
    grid holds, so `>=` against `>` decides."""
    case = lattices[f"min-weight-{min_weight}"]
    weight = case[0][1]
    assert (weight == np.float32(min_weight)).sum() > 100 and np.isnan(weight).sum() > 100
    nV, nT, _, _ = _assert_extraction(case, f"min_weight {min_weight}")
    assert nT > 500


def test_every_corner_configuration_once(lattices):
    assert _assert_extraction(lattices["configs"], "configs")[:2] == (2432, 1920)


@pytest.mark.parametrize("name", ["x".join(map(str, d)) for d in SMALL_DIMS])
def test_small_and_ragged_dimensions(lattices, name):
    """Dimensions at the minimum of 2 in one, two and three axes; 65 x 2 x 3 and 2 x 257 x 2 end a row one node into the next wave and
    the next block."""
    nV, nT, _, _ = _assert_extraction(lattices[name], name)
    assert nT > 0


@pytest.mark.parametrize("name", ["2x2x2-all-inside", "2x2x2-one-corner-zero", "2x2x2-one-corner-nan", "2x2x2-one-corner-half"])
def test_one_cell_that_gives_nothing(lattices, name):
    """A single cell with every node inside, and with one corner invalid (weight 0, NaN, or below min_weight): an empty mesh."""
    assert _assert_extraction(lattices[name], name)[:2] == (0, 0)


def test_long_column_beyond_the_first_round_of_the_scan(lattices):
    """6 x 5 x 10022 nodes, 1175 blocks: scan_spine_kernel scans 1024 block sums per round, so blocks 1024 to 1174 get their bases from the
    64-bit carries of a second round, and 47 % of the faces lie there (tests/test_mesh_ref.py holds the fixture to that).  A lost or
    truncated carry moves every vertex row and face index behind node 262 144."""
    case = lattices["column"]
    nodes = int(np.prod(case[1]))
    assert -(-nodes // 256) > 1024 + 100
    nV, nT, _, _ = _assert_extraction(case, "column")
    assert nV > 2 ** 17 and nT > 2 ** 18


# ------------------------------------------------------------------------------------------------- streams
def test_integrate_then_extract_on_a_side_stream_behind_a_producer(views):
    """The depth map is produced on the side stream right in front of integrate, extract follows, and the host does not wait in between:
    equal to the default-stream result."""
    def run(stream):
        vol = _volume()
        inputs = [_stage(vw) for vw in views]
        big = torch.randn(4_000_000, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())            # the zero fill and the uploads above ran on the default stream
        with torch.cuda.stream(stream):
            for vw, (staged, cam, rgb, alpha) in zip(views, inputs):
                for _ in range(4):
                    big = big * 1.0001 + 0.5                       # keeps the stream busy in front of the producer
                depth = staged * 0.5
                depth.mul_(2.0)                                    # the producer: integrate must see its result (exact: a power of two)
                _integrate(vol, vw, staged=(depth, cam, rgb, alpha))
            mesh = vol.extract()
        stream.synchronize()
        return vol, mesh
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    vol_s, mesh_s = run(side)
    vol_d, mesh_d = run(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for name in ("tsdf", "weight", "color"):
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


def end_to_end():
    """(mesh, extractor, median | |v| - R | of the device's mesh, the same of the restatement on the downloaded maps)."""
    import gsr_synth as S
    from gaussian_renderer import render
    from utils.mesh_utils import GaussianExtractor
    PC, Pipe = _ball_model()
    cams = S.circle_cameras(96, 64, n=6)
    ex = GaussianExtractor(PC, render, Pipe)
    ex.reconstruction([cameras.view_of(c) for c in cams])
    mesh = ex.extract_mesh_bounded(voxel_size=0.05, sdf_trunc=0.2, depth_trunc=10)
    v = mesh.vertices.cpu().numpy().astype(np.float64)
    # the restatement on the downloaded maps, over the volume extract_mesh_bounded lays out (origin and voxel as the device gets them)
    centre, radius = ex.camera_bounds()
    lo = [float(c) - radius for c in centre]
    dims = tuple(max(2, int(np.ceil(2 * radius / 0.05)) + 1) for _ in range(3))
    ref = M.Volume(dims, lo, 0.05, color=False)
    for cam, depth, alpha in zip(cams, ex.depthmaps, ex.alphamaps):
        M.integrate(ref, depth[0].cpu().numpy(), None, alpha[0].cpu().numpy(), 0.5, cam["viewmatrix"], cam["projmatrix"], 0.2, 10.0)
    vr = M.extract_vertices(ref.tsdf.astype(np.float32), ref.weight.astype(np.float32), ref.origin.astype(np.float64), ref.voxel)
    stat = lambda p: float(np.median(np.abs(np.linalg.norm(p, axis=1) - BALL_RADIUS)))
    return mesh, ex, stat(v), stat(vr), len(vr)


def test_gaussian_extractor_end_to_end(tmp_path):
    import gsr_mesh
    mesh, ex, device, reference, ref_vertices = end_to_end()
    print(f"end to end: {mesh.vertices.shape[0]} vertices ({ref_vertices} in the restatement), {mesh.faces.shape[0]} faces, "
          f"median | |v| - R |: device {device:.4f}, restatement {reference:.4f}")
    assert mesh.vertices.shape[0] > 1000 and mesh.faces.shape[0] > 1000
    assert len(ex.depthmaps) == len(ex.normals) == 6 and all(t.is_cuda for t in ex.depthmaps + ex.alphamaps + ex.rgbmaps + ex.normals)
    assert torch.allclose(ex.normals[0].norm(dim=0)[ex.alphamaps[0][0] > 0.5], torch.tensor(1.0, device="cuda"), atol=1e-4)
    assert int(mesh.faces.max()) == mesh.vertices.shape[0] - 1 and int(mesh.faces.min()) == 0
    assert abs(mesh.vertices.shape[0] - ref_vertices) <= 0.01 * ref_vertices      # (float32 may class a node at tsdf ~ 0 differently)
    assert device <= 2 * reference
    path = tmp_path / "ball.ply"
    gsr_mesh.save_mesh_ply(str(path), mesh)
    v, c, f = M.read_ply(str(path))
    assert (v == mesh.vertices.cpu().numpy()).all() and (f == mesh.faces.cpu().numpy()).all() and c.shape == v.shape
    t = M.topology(f, len(v))
    assert t["unreferenced"] == 0 and t["nonmanifold"] == 0 and t["repeated_directed"] == 0


def gpu_mesh_figures():
    """The figures the constants at the top record, for a measurement run."""
    views = M.integrate_fixture()
    out = dict(integrate=integrate_errors(views, M.integrate_reference(views)),
               extract=extract_errors({name: (make(), M.extract(*make(), M.GRID_ORIGIN, M.GRID_VOXEL)) for name, make in GRIDS.items()}))
    mesh, _, device, reference, nref = end_to_end()
    out["end_to_end"] = dict(device=device, reference=reference, device_vertices=int(mesh.vertices.shape[0]), reference_vertices=nref)
    return out
