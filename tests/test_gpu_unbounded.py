"""The unbounded mesh extraction on the GPU against the float64 restatement (tests/unbounded_ref.py): TSDF integration into a lattice in
contracted space over one, two and three views, the rule that a skipped element is not written, per-vertex colouring, the un-contraction
of points, stream ordering, and the three Python layers end to end (gsr_mesh.ContractedTSDFVolume, GaussianExtractor.extract_mesh_unbounded,
utils.mcube_utils.marching_cubes_with_contraction).

Tolerances.  The restatement is float64 on the float32 inputs, so what is compared is the device's float32 rounding.  Each tolerance is
four times the largest error observed on an MI355X against the restatement (gpu_unbounded_figures() prints the figures; DESIGN.md, "Mesh
extraction" records them), the margin tests/test_gpu_mesh.py uses and for its reason: the compiler is free to contract a multiply and an
add into an fma, which moves a few ulps through the divisions, while a wrong pixel convention, a wrong tap or a transposed matrix is off
by orders of magnitude.  The un-contraction does not use an observed figure: its bound per coordinate follows from the kernel's arithmetic
(uncontract_bound).
"""
import numpy as np
import pytest
import torch

import cameras
import mesh_ref as M
import poison
import unbounded_ref as U

pytestmark = pytest.mark.gpu

# largest |device - restatement| observed on an MI355X, and the tolerances that follow
# (larger than the bounded volume's 3.2e-7: beyond the unit ball the world position divides by 2 - m, which carries m's rounding m / (2 - m)
# times as large, and the fixture's plane is written out to m = 1.7; the colours are random per pixel, so a tap weight's rounding counts in full)
CONTRACTED_OBSERVED = {"tsdf": 7.93e-6}     # over both lattices and the fixture's three views (the 33^3 lattice after one view)
POINTS_OBSERVED = {"color": 4.15e-6}        # 5000 points, three views
CONTRACTED_TOL = {k: 4 * v for k, v in CONTRACTED_OBSERVED.items()}
POINTS_TOL = {k: 4 * v for k, v in POINTS_OBSERVED.items()}
UNCONTRACT_OBSERVED = 0.538                 # largest |device - restatement| / uncontract_bound (the test prints its own)
# end to end: median distance of the vertices inside the unit ball to the analytic surface as observed, device and float64 restatement
# (14986 vertices each, 3204 of them inside the unit ball); the test allows the device twice the restatement's figure of its run
E2E_OBSERVED = {"reference": 0.046817, "device": 0.046817}
GUARD = 64                                  # floats in front of and behind each guarded plane
POINTS_SDF_TRUNC = 0.15
E2E_RESOLUTION, E2E_EXTENT, E2E_ROUNDS = 48, 1.9, 4


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _guarded(shape, pattern, dtype=torch.float32):
    """(buffer, view of `shape` inside it): every byte of the buffer is `pattern`; GUARD elements lie on either side of the view."""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 2 * GUARD, dtype=dtype, device="cuda")
    buf.view(torch.uint8).fill_(pattern)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _assert_guards(bufs, pattern):
    word = np.uint32(pattern * 0x01010101)
    for buf in bufs:
        raw = poison.u32(buf.cpu().numpy())
        assert (raw[:GUARD] == word).all() and (raw[-GUARD:] == word).all()


def _lattice(n, extent, centre=U.FIX_CENTRE, radius=U.FIX_RADIUS, pattern=None):
    """A ContractedTSDFVolume; with `pattern`, its planes are views into guarded buffers filled with it (returned as .guards)."""
    import gsr_mesh
    vol = gsr_mesh.ContractedTSDFVolume(centre, radius, n, extent, "cuda")
    vol.guards = []
    if pattern is not None:
        for name in ("tsdf", "weight"):
            buf, view = _guarded((n, n, n), pattern)
            setattr(vol, name, view)
            vol.guards.append(buf)
    return vol


def _stage(vw):
    """The view's inputs on the device: (camera object, depth, rgb)."""
    return cameras.view_of(vw["cam"]), _dev(vw["depth"]), _dev(vw["rgb"])


@pytest.fixture(scope="module")
def views():
    return M.integrate_fixture()


@pytest.fixture(scope="module")
def references(views):
    return {(n, extent): U.fixture_reference(n, extent, views) for n, extent in U.FIX_LATTICES}


# ------------------------------------------------------------------------------------------------- integration
def contracted_errors(n, extent, views, reference):
    """Per number of views: largest |device - restatement| of tsdf over the stable nodes, and whether weight is exact there."""
    vol = _lattice(n, extent)
    out = []
    for vw, (tsdf, weight, _, unstable) in zip(views, reference):
        cam, depth, _ = _stage(vw)
        vol.integrate(depth, cam)
        ok = ~unstable
        out.append(dict(tsdf=float(np.abs(vol.tsdf.cpu().numpy() - tsdf)[ok].max()), weight_exact=bool((vol.weight.cpu().numpy() == weight)[ok].all()),
                        stable=int(ok.sum())))
    return out


@pytest.mark.parametrize("n, extent", U.FIX_LATTICES)
def test_integrate_parity_after_one_two_and_three_views(views, references, n, extent):
    for k, e in enumerate(contracted_errors(n, extent, views, references[(n, extent)])):
        print(f"n {n} extent {extent} views {k + 1}: tsdf {e['tsdf']:.3e} over {e['stable']} stable nodes")
        assert e["weight_exact"], k
        assert e["stable"] >= 0.99 * n ** 3
        assert e["tsdf"] <= CONTRACTED_TOL["tsdf"], (k, e)


def test_integrate_takes_a_depth_map_with_a_channel_axis_and_reset_starts_over(views, references):
    n, extent = U.FIX_LATTICES[1]
    tsdf, weight, _, unstable = references[(n, extent)][0]
    vol = _lattice(n, extent)
    cam, depth, _ = _stage(views[0])
    vol.integrate(depth[None], cam)
    first = vol.tsdf.clone()
    assert (vol.weight.cpu().numpy() == weight)[~unstable].all()
    vol.integrate(depth, cam)
    vol.reset()
    assert float(vol.tsdf.min()) == 1.0 == float(vol.tsdf.max()) and float(vol.weight.min()) == 1.0 == float(vol.weight.max())
    vol.integrate(depth, cam)
    assert torch.equal(vol.tsdf, first)
    with pytest.raises(ValueError, match="depth must be"):
        vol.integrate(depth[:, :-1], cam)
    with pytest.raises(ValueError, match="is on cpu"):
        vol.integrate(depth.cpu(), cam)


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=lambda p: "0x%02X" % p)
def test_a_skipped_node_is_not_written_and_the_guard_bands_stay(views, references, pattern):
    """Every node no view has written so far, every node beyond the shell among them, keeps the bytes it had."""
    n, extent = U.FIX_LATTICES[0]
    vol = _lattice(n, extent, pattern=pattern)
    word = np.uint32(pattern * 0x01010101)
    m = np.linalg.norm(U.Lattice(n, extent, U.FIX_CENTRE, U.FIX_RADIUS).nodes(), axis=-1)
    written_any = np.zeros((n, n, n), bool)
    for vw, (_, _, written, unstable) in zip(views, references[(n, extent)]):
        cam, depth, _ = _stage(vw)
        vol.integrate(depth, cam)
        written_any |= written
        keep = ~written_any & ~unstable
        assert keep.sum() > 0.5 * keep.size and (keep & (m >= 2)).sum() > 15000 and (keep & (m < 2)).sum() > 10000
        for name in ("tsdf", "weight"):
            assert (poison.u32(getattr(vol, name).cpu().numpy())[keep] == word).all(), name
        if pattern != 0xFF:                     # 0 or 2.4e-38 as the previous weight: the view's own nodes were written
            assert (vol.weight.cpu().numpy()[written & ~unstable] >= 1).all()
    _assert_guards(vol.guards, pattern)


# ------------------------------------------------------------------------------------------------- per-vertex colours
def _fuse_points(points, views, color, weight):
    from _gsr import check, lib, ptr, stream_ptr
    for vw in views:
        cam, depth, rgb = _stage(vw)
        check(lib.gsr_points_fuse_view(ptr(points), points.shape[0], ptr(color), ptr(weight), ptr(depth), ptr(rgb), vw["cam"]["W"], vw["cam"]["H"],
                                       ptr(cam.world_view_transform), ptr(cam.full_proj_transform), POINTS_SDF_TRUNC, stream_ptr("cuda")),
              "gsr_points_fuse_view")


@pytest.fixture(scope="module")
def points_reference(views):
    """(points float32, color f64, weight f64, [written per view], unstable) of the restatement over the three views."""
    pts = U.fixture_points()
    color, weight = np.zeros((len(pts), 3)), np.zeros(len(pts))
    unstable, written = np.zeros(len(pts), bool), []
    for vw in views:
        w, uns = U.fuse_points(pts, color, weight, vw["depth"], vw["rgb"], vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"], POINTS_SDF_TRUNC)
        written.append(w)
        unstable |= uns
    return pts, color, weight, written, unstable


def points_errors(views, points_reference):
    import gsr_mesh
    pts, color, weight, _, unstable = points_reference
    got = gsr_mesh.color_vertices(_dev(pts), [_stage(vw) for vw in views], POINTS_SDF_TRUNC)
    ok = ~unstable
    # the weights are not returned by the Python layer: the raw entry, from the same fresh state
    c2, w2 = torch.zeros((len(pts), 3), device="cuda"), torch.zeros(len(pts), device="cuda")
    _fuse_points(_dev(pts), views, c2, w2)
    return dict(color=float(np.abs(got.cpu().numpy() - color)[ok].max()), weight_exact=bool((w2.cpu().numpy() == weight)[ok].all()),
                same_bytes=bool(torch.equal(got, c2)), stable=int(ok.sum()), seen=int((weight > 0).sum()))


def test_points_fuse_view_parity(views, points_reference):
    e = points_errors(views, points_reference)
    print(f"points: colour {e['color']:.3e} over {e['stable']} stable points, {e['seen']} seen by a view")
    assert e["weight_exact"] and e["same_bytes"]
    assert e["stable"] >= 0.99 * 5000 and e["seen"] > 1500
    assert e["color"] <= POINTS_TOL["color"], e


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=lambda p: "0x%02X" % p)
def test_a_skipped_point_is_not_written(views, points_reference, pattern):
    pts, _, _, written, unstable = points_reference
    word = np.uint32(pattern * 0x01010101)
    cbuf, color = _guarded((len(pts), 3), pattern)
    wbuf, weight = _guarded((len(pts),), pattern)
    points = _dev(pts)
    seen = np.zeros(len(pts), bool)
    for vw, w in zip(views, written):
        _fuse_points(points, [vw], color, weight)
        seen |= w
        keep = ~seen & ~unstable
        assert keep.sum() > 1000
        assert (poison.u32(weight.cpu().numpy())[keep] == word).all() and (poison.u32(color.cpu().numpy())[keep] == word).all()
        if pattern != 0xFF:
            assert (weight.cpu().numpy()[w & ~unstable] >= 1).all()
    _assert_guards([cbuf, wbuf], pattern)
    assert torch.equal(points, _dev(pts))


def test_color_vertices_of_no_vertices_and_of_no_views(views):
    import gsr_mesh
    none = gsr_mesh.color_vertices(torch.empty((0, 3), device="cuda"), [_stage(views[0])], POINTS_SDF_TRUNC)
    assert none.shape == (0, 3) and none.dtype == torch.float32
    black = gsr_mesh.color_vertices(_dev(U.fixture_points(10)), [], POINTS_SDF_TRUNC)
    assert black.shape == (10, 3) and float(black.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------- un-contraction
UNC_CENTRE, UNC_RADIUS, UNC_RANGE = (-0.2, 0.1, 0.8), 0.5, 32.0


def uncontract_points_fixture():
    """Contracted points float32 [2005, 3]: 1000 in the unit ball, 1000 in the shell up to m = 1.95, and five special ones: on the shell's
    outer sphere, beyond it, far beyond it, one whose world position lies beyond max_range along x, and the centre."""
    rs = np.random.RandomState(12)
    d = rs.randn(2000, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = np.concatenate([rs.uniform(0.0, 0.999, 1000), rs.uniform(1.001, 1.95, 1000)])
    special = [[0.0, 2.0, 0.0], [1.5, -1.5, 0.5], [-40.0, 3.0, 9.0], [1.995, 0.0, 0.0], [0.0, 0.0, 0.0]]
    return np.concatenate([d * m[:, None], special]).astype(np.float32)


def uncontract_bound(src, want):
    """The bound on |device - restatement| per coordinate that follows from the kernel's arithmetic and not from its results: m is a sum
    of three products and a square root (at most four roundings), 2 - m inherits m's absolute error, which is m / (2 - m) times as
    large relative to it, the product, the reciprocal and the scale by the radius add three more, and the fma that forms c + s y
    rounds once: (8 + 4 m / (2 - m)) roundings of |s y| and one of the result."""
    y = src.astype(np.float64)
    m = np.linalg.norm(y, axis=1, keepdims=True)
    term = np.abs(UNC_RADIUS * y * U.uncontract_scale(m))
    return M.U32 * (np.abs(want) + term * (8 + 4 * m / (2 - m)))


def uncontract_errors():
    from _gsr import check, lib, ptr, stream_ptr
    src = uncontract_points_fixture()
    want = U.uncontract_points(src, UNC_CENTRE, UNC_RADIUS, UNC_RANGE)
    buf = _dev(src)
    check(lib.gsr_uncontract_points(ptr(buf), ptr(buf), len(src), *UNC_CENTRE, UNC_RADIUS, UNC_RANGE, stream_ptr("cuda")), "gsr_uncontract_points")
    return src, want, buf.cpu().numpy()


def test_uncontract_points_in_place():
    src, want, got = uncontract_errors()
    m = np.linalg.norm(src.astype(np.float64), axis=1)
    ball, shell = m < 1, (m > 1) & (m < 1.96)
    assert ball.sum() == 1001 and shell.sum() == 1000
    assert np.array_equal(got[ball], want[ball].astype(np.float32))                      # one fma: the float64 result, rounded once
    ratio = float((np.abs(got[shell] - want[shell]) / uncontract_bound(src[shell], want[shell])).max())
    print(f"uncontract: |device - restatement| / bound {ratio:.3f} over {int(shell.sum())} shell points (coordinates up to {np.abs(want[shell]).max():.1f})")
    assert ratio <= 1.0
    assert np.isfinite(got).all() and np.abs(got).max() <= UNC_RANGE
    # m >= 2: the scale of the largest float32 below 2 (4.2e6), clipped wherever the coordinate is not zero
    assert np.array_equal(got[2000], np.array([UNC_CENTRE[0], UNC_RANGE, UNC_CENTRE[2]], np.float32))
    assert np.array_equal(got[2001], np.array([UNC_RANGE, -UNC_RANGE, UNC_RANGE], np.float32))
    assert np.array_equal(got[2002], np.array([-UNC_RANGE, UNC_RANGE, UNC_RANGE], np.float32))
    # m = 1.995: x = 0.5 * 1.995 / (1.995 * 0.005) = 100 beyond the centre, clipped to max_range; y and z stay at the centre
    assert np.array_equal(got[2003], np.array([UNC_RANGE, UNC_CENTRE[1], UNC_CENTRE[2]], np.float32))
    assert np.array_equal(got[2004], np.array(UNC_CENTRE, np.float32))


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=lambda p: "0x%02X" % p)
def test_uncontract_points_writes_its_rows_and_nothing_else(pattern):
    from _gsr import check, lib, ptr, stream_ptr
    src = uncontract_points_fixture()
    _, want, in_place = uncontract_errors()
    source = _dev(src)
    buf, dst = _guarded((len(src) + 7, 3), pattern)
    check(lib.gsr_uncontract_points(ptr(source), ptr(dst), len(src), *UNC_CENTRE, UNC_RADIUS, UNC_RANGE, stream_ptr("cuda")), "gsr_uncontract_points")
    assert np.array_equal(dst[:len(src)].cpu().numpy(), in_place)                         # dst != src gives what dst == src gives
    assert (poison.u32(dst[len(src):].cpu().numpy()) == np.uint32(pattern * 0x01010101)).all()
    _assert_guards([buf], pattern)
    assert torch.equal(source, _dev(src))


# ------------------------------------------------------------------------------------------------- streams
def test_integrate_then_extract_on_a_side_stream_behind_a_producer(views):
    """The depth map is produced on the side stream right in front of integrate, extract and the colouring follow, and the host does not
    wait in between: equal to the default-stream result."""
    import gsr_mesh
    n, extent = U.FIX_LATTICES[0]

    def run(stream):
        vol = _lattice(n, extent)
        inputs = [_stage(vw) for vw in views]
        big = torch.randn(4_000_000, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())            # the fill and the uploads above ran on the default stream
        with torch.cuda.stream(stream):
            produced = []
            for _ in range(2):                                     # twice: a node needs two observations to outweigh the fresh state
                for cam, staged, rgb in inputs:
                    for _ in range(4):
                        big = big * 1.0001 + 0.5                   # keeps the stream busy in front of the producer
                    depth = staged * 0.5
                    depth.mul_(2.0)                                # the producer: integrate must see its result (exact: a power of two)
                    vol.integrate(depth, cam)
                    produced.append((cam, depth, rgb))
            mesh = vol.extract()
            colors = gsr_mesh.color_vertices(mesh.vertices, produced[:3], 5.0 * vol.voxel_size)
        stream.synchronize()
        return vol, mesh, colors
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    vol_s, mesh_s, colors_s = run(side)
    vol_d, mesh_d, colors_d = run(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for name in ("tsdf", "weight"):
        assert torch.equal(getattr(vol_s, name), getattr(vol_d, name)), name
    assert mesh_s.vertices.shape[0] > 0 and mesh_s.colors is None and float(colors_s.abs().sum()) > 0
    assert torch.equal(mesh_s.vertices, mesh_d.vertices) and torch.equal(mesh_s.faces, mesh_d.faces) and torch.equal(colors_s, colors_d)


# ------------------------------------------------------------------------------------------------- end to end, analytic
def end_to_end():
    """(mesh, median distance to the analytic surface of the device's vertices inside the unit ball, the same of the restatement, the
    restatement's vertex count): the ball in front of the endless floor (unbounded_ref.ball_scene), each of the six views fused
    E2E_ROUNDS times (a node needs more than one observation to outweigh the fresh volume's free space)."""
    scene = U.ball_scene()
    vol = _lattice(E2E_RESOLUTION, E2E_EXTENT, U.BALL_CENTRE, U.BALL_RADIUS)
    ref = U.Lattice(E2E_RESOLUTION, E2E_EXTENT, U.BALL_CENTRE, U.BALL_RADIUS)
    staged = [(cameras.view_of(cam), _dev(depth)) for cam, depth in scene]
    for _ in range(E2E_ROUNDS):
        for (cam, depth), (view, ddepth) in zip(scene, staged):
            vol.integrate(ddepth, view)
            U.integrate(ref, depth, cam["viewmatrix"], cam["projmatrix"])
    mesh = vol.extract()
    yr = M.extract_vertices(ref.tsdf.astype(np.float32), ref.weight.astype(np.float32), (ref.lo,) * 3, ref.step)
    vr = U.uncontract_points(yr, U.BALL_CENTRE, U.BALL_RADIUS, 32.0)
    v = mesh.vertices.cpu().numpy().astype(np.float64)

    def stat(p):
        inside = np.linalg.norm(p - np.asarray(U.BALL_CENTRE), axis=1) < U.BALL_RADIUS
        return float(np.median(U.ball_distance(p[inside]))), int(inside.sum())
    return mesh, stat(v), stat(vr), len(vr)


def test_contracted_volume_end_to_end_on_an_analytic_scene():
    mesh, (device, device_inside), (reference, reference_inside), ref_vertices = end_to_end()
    nV, nT = mesh.vertices.shape[0], mesh.faces.shape[0]
    print(f"end to end: {nV} vertices ({ref_vertices} in the restatement), {nT} faces, {device_inside} ({reference_inside}) inside the unit ball, "
          f"median distance to the surface: device {device:.5f}, restatement {reference:.5f}")
    assert nV > 1000 and nT > 2000 and device_inside > 300 and nV - device_inside > 300
    assert mesh.colors is None and mesh.faces.dtype == torch.int32 and mesh.vertices.is_cuda
    assert abs(nV - ref_vertices) <= 0.01 * ref_vertices           # (float32 may class a node at tsdf ~ 0 differently)
    t = M.topology(mesh.faces.cpu().numpy(), nV)
    assert t["boundary"] == 0 and t["unreferenced"] == 0           # closed: the lattice's border is free space
    assert int(mesh.faces.max()) == nV - 1 and int(mesh.faces.min()) == 0
    assert float(mesh.vertices.abs().max()) <= 32.0
    assert device <= 2 * reference
    assert reference <= 0.5 * 2 * U.BALL_RADIUS / E2E_RESOLUTION * 5   # and the restatement itself lies within half the truncation of the surface


# ------------------------------------------------------------------------------------------------- GaussianExtractor
def _surfel_model():
    """The ball of surfels of tests/test_gpu_mesh.py with colours the renderer keeps inside [0.2, 0.8]: constant SH terms only, no
    reflection."""
    from test_gpu_mesh import _ball_model
    PC, Pipe = _ball_model()
    rs = np.random.RandomState(2)
    with torch.no_grad():
        PC.get_features.zero_()
        PC.get_features[:, 0] = _dev((rs.uniform(0.2, 0.8, (PC.get_features.shape[0], 3)) - 0.5) / 0.28209479177387814)
        PC.get_refl.zero_()
    return PC, Pipe


def test_gaussian_extractor_extract_mesh_unbounded():
    import gsr_mesh
    import gsr_synth as S
    from gaussian_renderer import render
    from utils.mesh_utils import GaussianExtractor
    PC, Pipe = _surfel_model()
    ex = GaussianExtractor(PC, render, Pipe)
    ex.reconstruction([cameras.view_of(c) for c in S.circle_cameras(96, 64, n=6)])
    mesh = ex.extract_mesh_unbounded(resolution=64)
    nV, nT = mesh.vertices.shape[0], mesh.faces.shape[0]
    rgb_lo, rgb_hi = min(float(r.min()) for r in ex.rgbmaps), max(float(r.max()) for r in ex.rgbmaps)
    print(f"extract_mesh_unbounded: {nV} vertices, {nT} faces, colours in [{float(mesh.colors.min()):.4f}, {float(mesh.colors.max()):.4f}], "
          f"rendered in [{rgb_lo:.4f}, {rgb_hi:.4f}], {int((mesh.colors.sum(1) > 0).sum())} vertices coloured")
    assert nV > 0 and nT > 0 and mesh.colors.shape == (nV, 3) and mesh.faces.dtype == torch.int32
    assert bool(torch.isfinite(mesh.colors).all()) and float(mesh.colors.min()) >= 0.0 and float(mesh.colors.max()) <= 1.0
    assert float(mesh.colors.max()) > 0
    assert bool(torch.isfinite(mesh.vertices).all()) and float(mesh.vertices.abs().max()) <= 32.0
    assert int(mesh.faces.max()) == nV - 1 and int(mesh.faces.min()) == 0
    # the extent: the 0.95 quantile of the contracted norms, numpy's default interpolation, in float64
    centre, radius = ex.camera_bounds()
    m = np.linalg.norm((PC.get_xyz.cpu().numpy().astype(np.float64) - centre.numpy()) / radius, axis=1)
    extent = ex.contracted_extent(centre, radius)
    assert abs(extent - min(float(np.quantile(np.where(m < 1, m, 2 - 1 / m), 0.95)) + 0.01, 1.9)) <= 1e-5
    # the hand-driven pipeline, bit for bit
    vol = gsr_mesh.ContractedTSDFVolume(centre, radius, 64, extent, "cuda")
    for cam, depth in zip(ex.viewpoint_stack, ex.depthmaps):
        vol.integrate(depth, cam)
    by_hand = vol.extract()
    colors = gsr_mesh.color_vertices(by_hand.vertices, zip(ex.viewpoint_stack, ex.depthmaps, ex.rgbmaps), 5.0 * vol.voxel_size)
    assert torch.equal(by_hand.vertices, mesh.vertices) and torch.equal(by_hand.faces, mesh.faces) and torch.equal(colors, mesh.colors)
    with pytest.raises(ValueError, match="reconstruction"):
        GaussianExtractor(PC, render, Pipe).extract_mesh_unbounded(resolution=8)


# ------------------------------------------------------------------------------------------------- marching_cubes_with_contraction
MC_RESOLUTION, MC_MIN, MC_SIDE = 32, (-1.2, -0.9, -1.1), 2.2


def test_marching_cubes_with_contraction_equals_the_restatement_face_by_face():
    from utils.mcube_utils import marching_cubes_with_contraction
    centre = torch.tensor([-0.13, 0.21, 0.07], device="cuda")
    seen = []

    def sdf(points):
        assert points.is_cuda and points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3 and points.shape[0] <= 256 ** 3
        seen.append((points - centre).norm(dim=1) - 0.77)
        return seen[-1]
    hi = tuple(c + MC_SIDE for c in MC_MIN)
    mesh = marching_cubes_with_contraction(sdf, resolution=MC_RESOLUTION, bounding_box_min=MC_MIN, bounding_box_max=hi, level=0.05)
    assert len(seen) == 1 and seen[0].shape == (MC_RESOLUTION ** 3,)
    values = (seen[0] - 0.05).cpu().numpy().reshape(MC_RESOLUTION, MC_RESOLUTION, MC_RESOLUTION)
    voxel = MC_SIDE / (MC_RESOLUTION - 1)
    V, _, F, ends = M.extract(values, np.ones_like(values), None, MC_MIN, voxel, ends=True)
    assert len(F) > 1000 and mesh.vertices.shape == (len(V), 3) and mesh.faces.shape == (len(F), 3) and mesh.colors is None
    assert (mesh.faces.cpu().numpy() == F).all()
    ratio = float((np.abs(mesh.vertices.cpu().numpy() - V) / M.extract_bounds(ends, voxel)[0]).max())
    print(f"marching_cubes_with_contraction: nV {len(V)} nT {len(F)}, |device - restatement| / bound {ratio:.3f}")
    assert ratio <= 1.0
    # the surface is the sphere of radius 0.77 + 0.05 about the centre, to the linear interpolation's error
    r = (mesh.vertices - centre).norm(dim=1)
    assert float((r - 0.82).abs().max()) <= 0.5 * voxel ** 2 / 0.82 * 3
    # with an inverse contraction: applied to the vertices, then the clip
    seen.clear()
    mapped = marching_cubes_with_contraction(sdf, MC_RESOLUTION, MC_MIN, hi, level=0.05, inv_contraction=lambda v: v * 3.0, max_range=2.0)
    assert torch.equal(mapped.faces, mesh.faces) and torch.equal(mapped.vertices, (mesh.vertices * 3.0).clamp(-2.0, 2.0))
    assert float(mapped.vertices.abs().max()) == 2.0


def gpu_unbounded_figures():
    """The figures the constants at the top record, for a measurement run."""
    views = M.integrate_fixture()
    out = dict(contracted={f"{n}-{extent}": contracted_errors(n, extent, views, U.fixture_reference(n, extent, views)) for n, extent in U.FIX_LATTICES})
    pts = U.fixture_points()
    color, weight, unstable, written = np.zeros((len(pts), 3)), np.zeros(len(pts)), np.zeros(len(pts), bool), []
    for vw in views:
        w, uns = U.fuse_points(pts, color, weight, vw["depth"], vw["rgb"], vw["cam"]["viewmatrix"], vw["cam"]["projmatrix"], POINTS_SDF_TRUNC)
        written.append(w)
        unstable |= uns
    out["points"] = points_errors(views, (pts, color, weight, written, unstable))
    src, want, got = uncontract_errors()
    m = np.linalg.norm(src.astype(np.float64), axis=1)
    shell = (m > 1) & (m < 1.96)
    out["uncontract"] = dict(ratio=float((np.abs(got[shell] - want[shell]) / uncontract_bound(src[shell], want[shell])).max()),
                             ball_exact=bool(np.array_equal(got[m < 1], want[m < 1].astype(np.float32))), specials=got[2000:].tolist())
    mesh, device, reference, nref = end_to_end()
    out["end_to_end"] = dict(device=device, reference=reference, device_vertices=int(mesh.vertices.shape[0]), reference_vertices=nref,
                             topology=M.topology(mesh.faces.cpu().numpy(), int(mesh.vertices.shape[0])))
    return out
