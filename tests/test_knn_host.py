"""simple_knn.distCUDA2 (csrc/gsr_knn.hip) on a machine without a GPU: the C entries are declared, exported and bound with the
header's argument lists, every refusal happens before any device work, the drop-in module imports and validates its input, and
gsr_init.load_point_cloud reads the reference's input clouds."""
import ctypes

import numpy as np
import pytest
import torch

GSR_E_INVALID = -1
FAKE = 0x7f0000000000          # 256-byte aligned, never dereferenced: every call below must fail validation first


@pytest.mark.parametrize("name, ret, args", [
    ("gsr_knn_scratch_bytes", "size_t", [ctypes.c_int]),
    ("gsr_knn_mean_dist", "int", [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
])
def test_knn_entries_are_declared_exported_and_bound(hip_lib_built, name, ret, args):
    """The two signatures, spelled out (tests/test_cabi.py holds every entry to its header and to the library's exports)."""
    import _gsr
    fn = getattr(_gsr.lib, name)
    assert list(fn.argtypes) == args
    assert fn.restype == (ctypes.c_size_t if ret == "size_t" else ctypes.c_int)


def test_scratch_bytes_covers_the_point_arrays(hip_lib_built):
    import _gsr
    f = _gsr.lib.gsr_knn_scratch_bytes
    assert f(0) == 0 and f(-1) == 0 and f(1 << 30) == 0
    for P in (1, 64, 65, 100_000):
        assert f(P) >= 28 * P          # Morton keys, sorted keys, order, sorted float4 points
    assert f(100_001) >= f(100_000)


@pytest.mark.parametrize("case, expect", [("negative", "P = -1"), ("too_many", "2^30"), ("points", "NULL"), ("out", "NULL"),
                                          ("scratch", "NULL"), ("scratch_small", "scratch of")])
def test_mean_dist_refuses_bad_arguments_before_any_device_call(hip_lib_built, case, expect):
    import _gsr
    P = 1000
    need = _gsr.lib.gsr_knn_scratch_bytes(P)
    a = dict(P=P, points=FAKE, out=FAKE, scratch=FAKE, nbytes=need, stream=None)
    a.update({"negative": dict(P=-1), "too_many": dict(P=1 << 30), "points": dict(points=None), "out": dict(out=None),
              "scratch": dict(scratch=None), "scratch_small": dict(nbytes=need - 1)}[case])
    rc = _gsr.lib.gsr_knn_mean_dist(*a.values())
    msg = _gsr.lib.gsr_last_error().decode()
    assert rc == GSR_E_INVALID, (case, rc, msg)
    assert msg.startswith("gsr_knn_mean_dist:") and expect in msg, (case, msg)


def test_empty_cloud_is_a_no_op(hip_lib_built):
    import _gsr
    assert _gsr.lib.gsr_knn_mean_dist(0, None, None, None, 0, None) == 0


def test_distcuda2_imports_as_the_reference_does(hip_lib_built):
    from simple_knn._C import distCUDA2
    import simple_knn
    assert callable(distCUDA2) and simple_knn._C.distCUDA2 is distCUDA2


def test_distcuda2_validates_its_input(hip_lib_built):
    """Shape, then dtype, then device: each check is reachable on a CPU tensor."""
    from simple_knn._C import distCUDA2
    with pytest.raises(ValueError, match="GPU"):
        distCUDA2(torch.zeros(10, 3))                              # a CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        distCUDA2(np.zeros((10, 3), np.float32))                   # not a tensor
    with pytest.raises(ValueError, match=r"\(P, 3\)"):
        distCUDA2(torch.zeros(10, 2))
    with pytest.raises(ValueError, match=r"\(P, 3\)"):
        distCUDA2(torch.zeros(30))
    with pytest.raises(RuntimeError, match="expected scalar type Float"):
        distCUDA2(torch.zeros(10, 3, dtype=torch.float64))


def _write_ply(path, points, rgb=None, normals=True):
    props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        props += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb is not None:
        props += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.zeros(points.shape[0], np.dtype(props))
    for i, n in enumerate("xyz"):
        v[n] = points[:, i]
    if rgb is not None:
        for i, n in enumerate(("red", "green", "blue")):
            v[n] = rgb[:, i]
    types = {"<f4": "float", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v) + "".join(
        "property %s %s\n" % (types[t], n) for n, t in props) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())


def test_load_point_cloud_with_colours(tmp_path, hip_lib_built):
    from gsr_init import load_point_cloud
    rs = np.random.RandomState(3)
    pts = rs.randn(500, 3).astype(np.float32)
    rgb = rs.randint(0, 256, (500, 3)).astype(np.uint8)
    path = str(tmp_path / "points3D.ply")
    _write_ply(path, pts, rgb)
    p, c = load_point_cloud(path)
    assert p.dtype == np.float32 and p.shape == (500, 3)
    np.testing.assert_array_equal(p, pts)
    assert c.dtype == np.float32 and c.shape == (500, 3)
    np.testing.assert_array_equal(c, (rgb / 255.0).astype(np.float32))


def test_load_point_cloud_without_colours(tmp_path, hip_lib_built):
    """fetchPly draws np.random.random((P, 3)) / 255 when the cloud has no colour; `seed` makes the draw reproducible."""
    from gsr_init import load_point_cloud
    pts = np.random.RandomState(4).rand(200, 3).astype(np.float32)
    path = str(tmp_path / "points3d.ply")
    _write_ply(path, pts, None, normals=False)
    p, c = load_point_cloud(path, seed=11)
    np.testing.assert_array_equal(p, pts)
    assert c.shape == (200, 3) and c.dtype == np.float32
    assert (c >= 0).all() and (c < 1.0 / 255.0).all()
    np.testing.assert_array_equal(c, (np.random.RandomState(11).random_sample((200, 3)) / 255.0).astype(np.float32))
    np.testing.assert_array_equal(load_point_cloud(path, seed=11)[1], c)
