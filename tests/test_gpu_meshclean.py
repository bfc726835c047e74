"""gsr_mesh.clean_mesh, cluster_connected_triangles and utils.mesh_utils.post_process_mesh on the GPU against the integer restatement
(tests/meshclean_ref.py).  Every comparison is exact: the label and size of every face, the six counts, the faces, and the rows of vertices
and colours bit for bit.  The shapes are the smallest that cross what can break: components that span several 256-blocks, the deepest
tree the union can build, more than 2^16 components (more than 256 blocks of roots), and the empty and all-ignored edges; component
sizes with a third byte and ties among them over more than 1024 blocks, 70 000 faces about one hub, a scrambled sheet, interleaved
chains, repeated faces."""
import numpy as np
import pytest
import torch

import cameras
import mesh_ref as M
import meshclean_ref as R
import poison

pytestmark = pytest.mark.gpu

ROW_GUARD = 16                   # rows behind every output
PARAMS = ((1, 50), (2, 50), (1000, 50), (1000, 0))          # (cluster_to_keep, min_triangles) of the two-sphere fixture


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _mesh(verts, faces, colors):
    import gsr_mesh
    return gsr_mesh.Mesh(_dev(verts, torch.float32), _dev(faces, torch.int32), None if colors is None else _dev(colors, torch.float32))


def _bits(t):
    return poison.u32(t.cpu().numpy())


def clean_raw(mesh, cluster_to_keep, min_triangles, pattern=0xFF):
    """gsr_mesh_clean_count + gsr_mesh_clean_emit called as clean_mesh calls them, on a scratch filled with `pattern` and with ROW_GUARD
    poisoned rows behind each output, which must come back untouched.  Returns a meshclean_ref.Cleaned of numpy arrays."""
    from _gsr import check, lib, ptr, stream_ptr
    nV, nT = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    scratch = torch.empty(int(lib.gsr_mesh_clean_scratch_bytes(nV, nT)), dtype=torch.uint8, device="cuda").fill_(pattern)
    counts = torch.full((6 + 2,), -3, dtype=torch.int64, device="cuda")
    tri_label = torch.full((nT + ROW_GUARD,), -7, dtype=torch.int32, device="cuda")
    tri_size = torch.full((nT + ROW_GUARD,), -7, dtype=torch.int32, device="cuda")
    check(lib.gsr_mesh_clean_count(ptr(mesh.faces), nV, nT, cluster_to_keep, min_triangles, ptr(tri_label), ptr(tri_size), ptr(scratch), scratch.numel(),
                                   ptr(counts), stream_ptr("cuda")), "gsr_mesh_clean_count")
    got = counts.tolist()
    assert got[6:] == [-3, -3]
    nV_out, nT_out = got[0], got[1]
    assert 0 <= nV_out <= nV and 0 <= nT_out <= nT
    verts = torch.full((nV_out + ROW_GUARD, 3), float("nan"), device="cuda")
    colors = None if mesh.colors is None else torch.full((nV_out + ROW_GUARD, 3), float("nan"), device="cuda")
    faces = torch.full((nT_out + ROW_GUARD, 3), -7, dtype=torch.int32, device="cuda")
    check(lib.gsr_mesh_clean_emit(ptr(mesh.vertices), ptr(mesh.colors), ptr(mesh.faces), nV, nT, ptr(scratch), ptr(verts), ptr(colors), ptr(faces),
                                  nV_out, nT_out, stream_ptr("cuda")), "gsr_mesh_clean_emit")
    assert (tri_label[nT:] == -7).all() and (tri_size[nT:] == -7).all()
    assert torch.isnan(verts[nV_out:]).all() and (faces[nT_out:] == -7).all() and (colors is None or torch.isnan(colors[nV_out:]).all())
    return R.Cleaned(verts[:nV_out].cpu().numpy(), faces[:nT_out].cpu().numpy(), None if colors is None else colors[:nV_out].cpu().numpy(),
                     tri_label[:nT].cpu().numpy(), tri_size[:nT].cpu().numpy(), tuple(got[:6]))


def assert_same(got, ref):
    """Every output, exactly; rows of floats by their bits."""
    assert tuple(got.counts) == tuple(ref.counts)
    assert got.tri_label.shape == ref.tri_label.shape and (got.tri_label == ref.tri_label).all()
    assert (got.tri_size == ref.tri_size).all()
    assert got.faces.shape == ref.faces.shape and (got.faces == ref.faces).all()
    assert got.verts.shape == ref.verts.shape and (poison.u32(got.verts) == poison.u32(ref.verts)).all()
    assert (got.colors is None) == (ref.colors is None)
    if ref.colors is not None:
        assert got.colors.shape == ref.colors.shape and (poison.u32(got.colors) == poison.u32(ref.colors)).all()


def via_python(mesh, cluster_to_keep, min_triangles):
    """The same through gsr_mesh's two functions."""
    import gsr_mesh
    out, info = gsr_mesh.clean_mesh(mesh, cluster_to_keep=cluster_to_keep, min_triangles=min_triangles, return_info=True)
    tri_label, tri_size = gsr_mesh.cluster_connected_triangles(mesh)
    assert out.faces.dtype == torch.int32 and out.vertices.is_cuda and tri_label.dtype == tri_size.dtype == torch.int32
    assert tuple(out.vertices.shape) == (info.vertices, 3) and tuple(out.faces.shape) == (info.faces, 3)
    return R.Cleaned(out.vertices.cpu().numpy(), out.faces.cpu().numpy(), None if out.colors is None else out.colors.cpu().numpy(),
                     tri_label.cpu().numpy(), tri_size.cpu().numpy(), tuple(info))


# ------------------------------------------------------------------------------------------------- spheres and floaters
@pytest.fixture(scope="module")
def spheres():
    """{"plain" | "scrambled": (verts, faces, colors, vertex labels)}: about 1.5 k faces per sphere, so a component spans several blocks;
    scrambled: faces in a random order, vertex rows permuted, so the hooking order and the labels differ."""
    verts, faces, colors, _ = R.two_spheres()
    out = {"plain": (verts, faces, colors), "scrambled": R.scrambled(verts, faces, colors, 21)}
    return {k: v + (R.vertex_labels(v[1], len(v[0])),) for k, v in out.items()}


@pytest.mark.parametrize("order", ["plain", "scrambled"])
@pytest.mark.parametrize("cluster_to_keep, min_triangles", PARAMS)
def test_spheres_and_floaters(spheres, order, cluster_to_keep, min_triangles):
    verts, faces, colors, labels = spheres[order]
    ref = R.clean(verts, faces, colors, cluster_to_keep, min_triangles, labels)
    mesh = _mesh(verts, faces, colors)
    assert_same(clean_raw(mesh, cluster_to_keep, min_triangles), ref)
    assert_same(via_python(mesh, cluster_to_keep, min_triangles), ref)
    if order == "scrambled":
        assert len(set(ref.tri_label.tolist())) == 2 + R.FLOATERS and ref.counts[2] == 2 + R.FLOATERS


def test_without_colours(spheres):
    verts, faces, _, labels = spheres["plain"]
    ref = R.clean(verts, faces, None, 1, 50, labels)
    assert_same(clean_raw(_mesh(verts, faces, None), 1, 50), ref)
    assert_same(via_python(_mesh(verts, faces, None), 1, 50), ref)
    assert ref.colors is None and ref.counts[1] > 1000


# ------------------------------------------------------------------------------------------------- the deepest tree
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_is_one_component(order):
    """Vertices 0..N and the faces (i, i+1, i+2), N = 2^16: hooked pair by pair this is a path of N links, the deepest tree there is."""
    N = 2 ** 16
    verts, faces, colors = R.chain(N - 1, order)
    assert len(verts) == N + 1
    got = clean_raw(_mesh(verts, faces, colors), 1, 50)
    assert got.counts == (N + 1, N - 1, 1, 1, N - 1, 0)
    assert (got.tri_label == 0).all() and (got.tri_size == N - 1).all()
    assert (got.faces == faces).all() and (poison.u32(got.verts) == poison.u32(verts)).all() and (poison.u32(got.colors) == poison.u32(colors)).all()


# ------------------------------------------------------------------------------------------------- many components
@pytest.fixture(scope="module")
def many():
    verts, faces, colors = R.singles()
    return verts, faces, colors, R.vertex_labels(faces, len(verts))


@pytest.mark.parametrize("min_triangles", [0, 50])
@pytest.mark.parametrize("cluster_to_keep", [1, 2, 70001, 10 ** 9])
def test_many_single_triangles(many, cluster_to_keep, min_triangles):
    """70 000 one-face components and one fan of 60: the k-th largest size is chosen across more than 256 blocks of roots; k = 2 lands in a
    70 000-way tie, 70 001 is the last component, 10^9 is clamped."""
    verts, faces, colors, labels = many
    ref = R.clean(verts, faces, colors, cluster_to_keep, min_triangles, labels)
    assert ref.counts[2] == 70001 and ref.counts[4] == max(60 if cluster_to_keep == 1 else 1, min_triangles)
    assert_same(clean_raw(_mesh(verts, faces, colors), cluster_to_keep, min_triangles), ref)


# ------------------------------------------------------------------------------------------------- edges
def test_empty_inputs(spheres):
    import gsr_mesh
    verts, faces, colors, _ = spheres["plain"]
    for v, f, c in ((verts, faces[:0], colors), (verts[:0], faces, colors[:0]), (verts[:0], faces[:0], None)):
        ref = R.clean(v, f, c, 3, 50)
        mesh = _mesh(v, f, c)
        assert_same(clean_raw(mesh, 3, 50), ref)
        assert_same(via_python(mesh, 3, 50), ref)
        out = gsr_mesh.clean_mesh(mesh)
        assert out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.faces.dtype == torch.int32 and (out.colors is None) == (c is None)


def test_bad_indices(spheres):
    """Faces with a repeated index, a negative index or one at or beyond nV: ignored, counted, and never used as an address."""
    verts, faces, colors, _ = spheres["plain"]
    nV = len(verts)
    bad = np.array([[5, 5, 9], [7, 8, 7], [3, 9, 9], [-1, 4, 5], [4, nV, 5], [4, 5, 2 ** 31 - 1], [-2 ** 31, 1, 2], [nV + 10 ** 6, 0, 1]], np.int32)
    mixed = np.concatenate([bad[:3], faces[:100], bad[3:], faces[100:]]).astype(np.int32)
    for f, k, m in ((mixed, 1, 50), (mixed, 1000, 0), (bad, 1, 0), (bad, 5, 7)):
        ref = R.clean(verts, f, colors, k, m)
        assert ref.counts[5] == len(bad)
        assert_same(clean_raw(_mesh(verts, f, colors), k, m), ref)
        assert_same(via_python(_mesh(verts, f, colors), k, m), ref)
    assert R.clean(verts, bad, colors, 5, 7).counts == (0, 0, 0, 0, 7, len(bad))


# ------------------------------------------------------------------------------------------------- what is not written, what does not matter
@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=lambda p: "0x%02X" % p)
def test_guard_bands_inputs_and_scratch_contents(spheres, pattern):
    """The scratch may hold anything beforehand; rows beyond nV_out and nT_out (clean_raw's guards) and the inputs are untouched; the
    Python layer's own allocations may hold anything too."""
    verts, faces, colors, labels = spheres["scrambled"]
    ref = R.clean(verts, faces, colors, 2, 50, labels)
    mesh = _mesh(verts, faces, colors)
    assert_same(clean_raw(mesh, 2, 50, pattern=pattern), ref)
    with poison.poisoned(pattern) as state:
        assert_same(via_python(mesh, 2, 50), ref)
    assert state.count >= 5
    assert (_bits(mesh.vertices) == poison.u32(verts)).all() and (_bits(mesh.colors) == poison.u32(colors)).all()
    assert (mesh.faces.cpu().numpy() == faces).all()


def test_two_calls_give_the_same_bytes(many, spheres):
    import gsr_mesh
    for verts, faces, colors, _ in (many, spheres["scrambled"]):
        mesh = _mesh(verts, faces, colors)
        runs = [(gsr_mesh.clean_mesh(mesh, cluster_to_keep=2, min_triangles=0, return_info=True), gsr_mesh.cluster_connected_triangles(mesh)) for _ in range(2)]
        ((a, ia), la), ((b, ib), lb) = runs
        assert ia == ib and torch.equal(a.faces, b.faces) and torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
        assert (_bits(a.vertices) == _bits(b.vertices)).all() and (_bits(a.colors) == _bits(b.colors)).all()


def test_on_a_side_stream_behind_a_producer(spheres):
    """The faces are produced on the side stream right in front of clean_mesh and the host does not wait in between."""
    import gsr_mesh
    verts, faces, colors, labels = spheres["scrambled"]
    ref = R.clean(verts, faces, colors, 1, 50, labels)
    staged = _mesh(verts, faces + 7, colors)
    big = torch.randn(4_000_000, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big * 1.0001 + 0.5                               # keeps the stream busy in front of the producer
        produced = staged.faces - 7                                 # the producer: clean_mesh must see its result
        out, info = gsr_mesh.clean_mesh(gsr_mesh.Mesh(staged.vertices, produced, staged.colors), cluster_to_keep=1, min_triangles=50, return_info=True)
        tri_label, tri_size = gsr_mesh.cluster_connected_triangles(gsr_mesh.Mesh(staged.vertices, produced, staged.colors))
    side.synchronize()
    assert_same(R.Cleaned(out.vertices.cpu().numpy(), out.faces.cpu().numpy(), out.colors.cpu().numpy(), tri_label.cpu().numpy(),
                          tri_size.cpu().numpy(), tuple(info)), ref)


# ------------------------------------------------------------------------------------------------- sizes of more than two bytes
STRIP_SIZES = (70000, 66000, 66000, 65536, 300, 256, 255, 1)          # 0x011170, 0x0101d0 twice, 0x010000: byte 2 is 1 in four of them
STRIP_PARAMS = tuple((k, 0) for k in range(1, 9)) + ((8, 65537), (2, 10 ** 9))


def _fixture(verts, faces, colors):
    """(verts, faces, colors, vertex labels, the mesh on the device)."""
    return verts, faces, colors, R.vertex_labels(faces, len(verts)), _mesh(verts, faces, colors)


@pytest.fixture(scope="module")
def strips():
    return _fixture(*R.scrambled(*R.strips(STRIP_SIZES), 31))


@pytest.mark.parametrize("cluster_to_keep, min_triangles", STRIP_PARAMS)
def test_sizes_with_a_third_byte(strips, cluster_to_keep, min_triangles):
    """Eight chains, four of them above 2^16 faces, scrambled: the select has to choose digit 1 in byte 2, then tell 0x11, 0x01, 0x01 and
    0x00 apart in byte 1 among the sizes that match, with a tie at 66 000 that k = 2 and k = 3 both land in.  268 348 faces and 268 364
    vertices are 1049 blocks of either, so the compaction's scan runs a second round too."""
    verts, faces, colors, labels, mesh = strips
    assert min(len(verts), len(faces)) > 1024 * 256
    ref = R.clean(verts, faces, colors, cluster_to_keep, min_triangles, labels)
    assert ref.counts[2] == 8 and ref.counts[4] == max(sorted(STRIP_SIZES, reverse=True)[cluster_to_keep - 1], min_triangles)
    assert_same(clean_raw(mesh, cluster_to_keep, min_triangles), ref)
    if (cluster_to_keep, min_triangles) == (3, 0):
        assert_same(via_python(mesh, cluster_to_keep, min_triangles), ref)
        assert ref.counts == R.clean(verts, faces, colors, 2, 0, labels).counts == (202006, 202000, 8, 3, 66000, 0)
    if cluster_to_keep == 4:
        assert ref.counts[1] == 70000 + 66000 + 66000 + 65536          # more than 2^18 kept faces: rows behind block 1023 move


# ------------------------------------------------------------------------------------------------- contention and shapes of the union
@pytest.fixture(scope="module")
def stars():
    out = {}
    for hub in ("first", "last"):
        plain = R.star(70000, hub)
        out[hub, "plain"] = _fixture(*plain)
        out[hub, "scrambled"] = _fixture(*R.scrambled(*plain, 33))
    return out


@pytest.mark.parametrize("order", ["plain", "scrambled"])
@pytest.mark.parametrize("hub", ["first", "last"])
def test_star_about_one_hub(stars, hub, order):
    """70 000 faces (hub, a_i, b_i) that share the hub only: every union names one address, as the root all arrive at (hub first) or as
    the vertex every thread tries to hang (hub last).  No two faces share an edge — connected by a vertex is connected here — and the one
    component has a third size byte."""
    verts, faces, colors, labels, mesh = stars[hub, order]
    ref = R.clean(verts, faces, colors, 1, 50, labels)
    assert ref.counts == (140001, 70000, 1, 1, 70000, 0) and len(set(ref.tri_label.tolist())) == 1
    assert_same(clean_raw(mesh, 1, 50), ref)
    assert_same(via_python(mesh, 1, 50), ref)
    assert_same(clean_raw(mesh, 2, 70001), R.clean(verts, faces, colors, 2, 70001, labels))          # nothing reaches the minimum


def test_scrambled_sheet():
    """A 300 x 300 grid of quads, 180 000 faces (0x02bf20) in one component, faces and vertex rows in random order: unions arrive from
    everywhere in a 2-D neighbourhood structure, not along a path."""
    verts, faces, colors, labels, mesh = _fixture(*R.scrambled(*R.sheet(300, 300), 32))
    ref = R.clean(verts, faces, colors, 1, 50, labels)
    assert ref.counts == (90601, 180000, 1, 1, 180000, 0)
    assert_same(clean_raw(mesh, 1, 50), ref)
    assert_same(via_python(mesh, 1, 50), ref)


@pytest.mark.parametrize("drop", [0, 1])
def test_interleaved_chains_stay_apart(drop):
    """Two chains of 40 000 faces on the even and the odd vertex indices: neighbouring indices never share a component, so a link to the
    wrong neighbour shows.  Equal sizes: k = 1 keeps both (the tie); one face fewer in the odd chain: k = 1 keeps the even one alone."""
    verts, faces, colors, labels, mesh = _fixture(*R.interleaved(40000, drop=drop))
    ref = R.clean(verts, faces, colors, 1, 0, labels)
    assert ref.counts == ((80004, 80000, 2, 2, 40000, 0) if drop == 0 else (40002, 40000, 2, 1, 40000, 0))
    assert sorted(set(ref.tri_label.tolist())) == [0, 1]
    assert_same(clean_raw(mesh, 1, 0), ref)
    assert_same(via_python(mesh, 1, 0), ref)
    assert_same(clean_raw(mesh, 2, 0), R.clean(verts, faces, colors, 2, 0, labels))


def test_repeated_faces_count_every_time():
    """Every third face said once more (as it is or rotated), scrambled: a repeat is a counted face, a component's size counts it, and
    the kept repeats are emitted."""
    verts, faces, colors, labels, mesh = _fixture(*R.scrambled(*R.with_duplicates(*R.strips((5000, 3000, 700, 2))), 34))
    assert len(faces) == 8702 + 2901
    for k, m in ((1, 0), (2, 0), (3, 1000), (4, 0)):
        ref = R.clean(verts, faces, colors, k, m, labels)
        assert_same(clean_raw(mesh, k, m), ref)
    assert ref.counts[1] == len(faces) and sorted(set(ref.tri_size.tolist())) == [3, 933, 4000, 6667]
    assert_same(via_python(mesh, 2, 0), R.clean(verts, faces, colors, 2, 0, labels))


# ------------------------------------------------------------------------------------------------- end to end
def _ball_model(P=4000, seed=1000, L=16):
    """The scene of tests/test_gpu_mesh.py's end-to-end test: random surfels about a ball."""
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


def test_post_process_mesh_end_to_end(tmp_path, capsys):
    import gsr_mesh
    import gsr_synth as S
    from gaussian_renderer import render
    from utils.mesh_utils import GaussianExtractor, post_process_mesh
    PC, Pipe = _ball_model()
    ex = GaussianExtractor(PC, render, Pipe)
    ex.reconstruction([cameras.view_of(c) for c in S.circle_cameras(96, 64, n=6)])
    mesh = ex.extract_mesh_bounded(voxel_size=0.1, sdf_trunc=0.4, depth_trunc=10)
    assert mesh.faces.shape[0] > 1000
    capsys.readouterr()
    out = post_process_mesh(mesh, cluster_to_keep=1)
    printed = capsys.readouterr().out.splitlines()
    assert printed[-2:] == [f"num vertices raw {mesh.vertices.shape[0]}", f"num vertices post {out.vertices.shape[0]}"]
    ref = R.clean(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.colors.cpu().numpy(), 1, 50)
    print(f"end to end: {mesh.faces.shape[0]} faces in {ref.counts[2]} components, the largest has {ref.counts[4]}; kept {ref.counts[1]} faces, "
          f"{ref.counts[0]} of {mesh.vertices.shape[0]} vertices")
    assert (out.faces.cpu().numpy() == ref.faces).all() and out.faces.shape == ref.faces.shape
    assert (_bits(out.vertices) == poison.u32(ref.verts)).all() and (_bits(out.colors) == poison.u32(ref.colors)).all()
    assert 0 < out.faces.shape[0] <= mesh.faces.shape[0]
    path = tmp_path / "ball_clean.ply"
    gsr_mesh.save_mesh_ply(str(path), out)
    v, c, f = M.read_ply(str(path))
    assert (poison.u32(v) == _bits(out.vertices)).all() and (f == out.faces.cpu().numpy()).all() and c.shape == v.shape
    assert M.topology(f, len(v))["unreferenced"] == 0
