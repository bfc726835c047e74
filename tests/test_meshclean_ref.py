"""tests/meshclean_ref.py, the restatement of include/gsr_hip_meshclean.h the GPU tests compare with, held to known answers: which sphere
stays under which parameters, the tie rule, the clamp, ignored faces, unreferenced vertices, and the closed surface of what is kept."""
import numpy as np
import pytest

import mesh_ref as M
import meshclean_ref as R


@pytest.fixture(scope="module")
def spheres():
    return R.two_spheres()


def test_labels_agree_with_scipy(spheres):
    verts, faces, _, _ = spheres
    by_scipy = R.labels_by_scipy(faces, len(verts))
    if by_scipy is None:
        pytest.skip("scipy is not installed")
    assert (R.vertex_labels(faces, len(verts)) == by_scipy).all()
    v, f, _ = R.scrambled(verts, faces, None, 3)
    assert (R.vertex_labels(f, len(v)) == R.labels_by_scipy(f, len(v))).all()


def test_cluster_to_keep_1_keeps_the_larger_sphere_only(spheres):
    verts, faces, colors, parts = spheres
    (nVa, nTa), (nVb, nTb) = parts["big"], parts["small"]
    out = R.clean(verts, faces, colors, 1, 50)
    assert out.counts == (nVa, nTa, 2 + R.FLOATERS, 1, nTa, 0)
    assert (out.verts == verts[2:2 + nVa]).all() and (out.colors == colors[2:2 + nVa]).all()
    assert (out.faces == faces[:nTa] - 2).all()                    # two unreferenced vertices in front vanish
    # labels: the smallest vertex index of each component; sizes: its faces
    assert (out.tri_label[:nTa] == 2).all() and (out.tri_size[:nTa] == nTa).all()
    assert (out.tri_label[nTa:nTa + nTb] == 2 + nVa).all() and (out.tri_size[nTa:nTa + nTb] == nTb).all()
    assert (out.tri_label[nTa + nTb:] == 2 + nVa + nVb + 3 * np.arange(R.FLOATERS)).all() and (out.tri_size[nTa + nTb:] == 1).all()
    # what is kept is still the closed sphere
    t = M.topology(out.faces, len(out.verts))
    assert t["boundary"] == 0 and t["nonmanifold"] == 0 and t["unreferenced"] == 0 and t["euler"] == 2


def test_cluster_to_keep_2_keeps_both(spheres):
    verts, faces, colors, parts = spheres
    (nVa, nTa), (nVb, nTb) = parts["big"], parts["small"]
    out = R.clean(verts, faces, colors, 2, 50)
    assert out.counts == (nVa + nVb, nTa + nTb, 2 + R.FLOATERS, 2, nTb, 0)
    assert (out.verts == verts[2:2 + nVa + nVb]).all() and (out.faces == faces[:nTa + nTb] - 2).all()


def test_min_triangles_drops_the_floaters_when_every_cluster_may_stay(spheres):
    verts, faces, colors, parts = spheres
    (nVa, nTa), (nVb, nTb) = parts["big"], parts["small"]
    out = R.clean(verts, faces, colors, 1000, 50)
    assert out.counts == (nVa + nVb, nTa + nTb, 2 + R.FLOATERS, 2, 50, 0)           # clamped to the 12 clusters: s_12 = 1, thr = 50
    everything = R.clean(verts, faces, colors, 1000, 0)
    assert everything.counts == (len(verts) - 5, len(faces), 2 + R.FLOATERS, 2 + R.FLOATERS, 1, 0)
    assert (everything.verts == verts[2:-3]).all() and (everything.faces == faces - 2).all() and (everything.colors == colors[2:-3]).all()


def test_ties_at_the_threshold_are_all_kept():
    verts, faces, colors = R.chain(40, "ascending")
    twice_v = np.concatenate([verts, verts + 1])
    twice_f = np.concatenate([faces, faces + len(verts)])
    out = R.clean(twice_v, twice_f, None, 1, 0)
    assert out.counts == (len(twice_v), len(twice_f), 2, 2, 40, 0) and out.colors is None
    assert (out.faces == twice_f).all() and (out.tri_label == np.repeat([0, len(verts)], 40)).all()


def test_bad_faces_are_ignored_and_counted(spheres):
    verts, faces, colors, parts = spheres
    nV = len(verts)
    bad = np.array([[5, 5, 9], [7, 8, 7], [3, 9, 9], [-1, 4, 5], [4, nV, 5], [4, 5, 2 ** 31 - 1], [-2 ** 31, 1, 2]], np.int32)
    mixed = np.concatenate([bad[:3], faces[:100], bad[3:], faces[100:]]).astype(np.int32)
    ref, out = R.clean(verts, faces, colors, 1, 50), R.clean(verts, mixed, colors, 1, 50)
    assert out.counts == ref.counts[:5] + (len(bad),)
    assert (out.faces == ref.faces).all() and (out.verts == ref.verts).all()
    ignored = np.r_[0:3, 103:107]
    assert (out.tri_label[ignored] == -1).all() and (out.tri_size[ignored] == 0).all()
    assert (np.delete(out.tri_label, ignored) == ref.tri_label).all()
    only_bad = R.clean(verts, bad, colors, 3, 7)
    assert only_bad.counts == (0, 0, 0, 0, 7, len(bad)) and only_bad.verts.shape == (0, 3) and only_bad.faces.shape == (0, 3)


def test_nothing_reaches_the_minimum_so_the_mesh_comes_back_empty():
    verts, faces, colors = R.chain(49, "shuffled")
    out = R.clean(verts, faces, colors, 1, 50)
    assert out.counts == (0, 0, 1, 0, 50, 0)
    assert out.verts.shape == (0, 3) and out.faces.shape == (0, 3) and out.colors.shape == (0, 3)
    assert (out.tri_label == 0).all() and (out.tri_size == 49).all()
    assert R.clean(verts, faces, colors, 1, 49).counts == (51, 49, 1, 1, 49, 0)


def test_empty_input():
    verts, faces, colors = R.chain(5, "ascending")
    assert R.clean(verts, faces[:0], colors, 1, 50).counts == (0, 0, 0, 0, 0, 0)
    out = R.clean(verts[:0], faces, None, 1, 50)
    assert out.counts == (0, 0, 0, 0, 0, 5) and (out.tri_label == -1).all() and (out.tri_size == 0).all()


def test_many_singles_select_clamp_and_tie():
    verts, faces, colors = R.singles()
    n, fan = 70000, 60
    assert R.clean(verts, faces, None, 1, 0).counts == (fan + 2, fan, n + 1, 1, fan, 0)
    assert R.clean(verts, faces, None, 2, 0).counts == (len(verts), n + fan, n + 1, n + 1, 1, 0)          # s_2 = 1: a 70 000-way tie
    assert R.clean(verts, faces, None, 2, 50).counts == (fan + 2, fan, n + 1, 1, 50, 0)
    assert R.clean(verts, faces, None, 10 ** 9, 0).counts == (len(verts), n + fan, n + 1, n + 1, 1, 0)   # the clamp


# ------------------------------------------------------------------------------------------------- the builders of the multi-byte and contention tests
def _labels(faces, nV):
    """vertex_labels(), held to scipy's where scipy is installed."""
    labels = R.vertex_labels(faces, nV)
    by_scipy = R.labels_by_scipy(faces, nV)
    assert by_scipy is None or (labels == by_scipy).all()
    return labels


def test_strips_have_the_sizes_asked_for():
    sizes = (700, 660, 660, 300, 256, 255, 1)
    verts, faces, colors = R.scrambled(*R.strips(sizes), 31)
    assert len(faces) == sum(sizes) and len(verts) == sum(sizes) + 2 * len(sizes)
    labels = _labels(faces, len(verts))
    assert sorted(np.bincount(labels[faces[:, 0]])[np.unique(labels)].tolist(), reverse=True) == sorted(sizes, reverse=True)
    thr = [R.clean(verts, faces, colors, k, 0, labels).counts[4] for k in range(1, len(sizes) + 1)]
    assert thr == [700, 660, 660, 300, 256, 255, 1]
    two, three = R.clean(verts, faces, colors, 2, 0, labels), R.clean(verts, faces, colors, 3, 0, labels)
    assert two.counts == three.counts == (700 + 660 + 660 + 6, 700 + 660 + 660, 7, 3, 660, 0) and (two.faces == three.faces).all()


def test_star_is_one_component_although_no_two_faces_share_an_edge():
    for hub in ("first", "last"):
        verts, faces, colors = R.star(500, hub)
        assert len(verts) == 1001 and (faces[:, 0] == (0 if hub == "first" else 1000)).all()
        assert M.topology(faces, len(verts))["boundary"] == 1500            # every edge lies in one face
        assert (_labels(faces, len(verts)) == 0).all()
        assert R.clean(verts, faces, colors, 1, 0).counts == (1001, 500, 1, 1, 500, 0)


def test_sheet_is_one_manifold_component():
    verts, faces, colors = R.sheet(30, 20)
    t = M.topology(faces, len(verts))
    assert (len(verts), len(faces)) == (31 * 21, 1200) and t["boundary"] == 100 and t["nonmanifold"] == 0 and t["euler"] == 1
    assert t["repeated_directed"] == 0 and t["unreferenced"] == 0
    v, f, _ = R.scrambled(verts, faces, colors, 32)
    assert (_labels(f, len(v)) == 0).all()


def test_interleaved_chains_stay_apart():
    verts, faces, colors = R.interleaved(400)
    labels = _labels(faces, len(verts))
    assert (labels == np.arange(len(verts)) % 2).all()
    assert R.clean(verts, faces, colors, 1, 0, labels).counts == (804, 800, 2, 2, 400, 0)          # the tie: k = 1 keeps both
    verts, faces, colors = R.interleaved(400, drop=1)
    out = R.clean(verts, faces, colors, 1, 0)
    assert out.counts == (402, 400, 2, 1, 400, 0) and (out.tri_size[1::2] == 399).all() and len(faces) == 799
    assert (out.verts == verts[::2]).all()


def test_repeated_faces_count_every_time():
    verts, faces, colors = R.strips((500, 300, 70, 2))
    v, f, c = R.with_duplicates(verts, faces, colors, every=3)
    assert len(f) == len(faces) + len(faces[::3])
    assert len(np.unique(np.sort(f, 1), axis=0)) == len(faces)                                     # nothing new, only repeats
    out = R.clean(v, f, c, 2, 0, _labels(f, len(v)))
    assert sorted(set(out.tri_size.tolist())) == [3, 93, 400, 667]                                  # 2 + 1, 70 + 23 (faces 800, 803, ...), 300 + 100, 500 + 167
    assert out.counts == (804, 1067, 4, 2, 400, 0)
