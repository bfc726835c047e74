"""simple_knn.distCUDA2 on the MI355X against an exact oracle: scipy's cKDTree in float64 on the same float32 coordinates, k = 4, the
smallest of the four (the point itself, or a duplicate at 0: the multiset is the same) dropped.  An exact float32 search is within a few
ulp of it (correctly rounded subtractions, three products and two sums), so 1e-6 relative (~8 ulp) per element; a single wrong
neighbour is orders of magnitude above that.  Zeros must be exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _oracle(pts):
    from scipy.spatial import cKDTree
    x = pts.astype(np.float64)
    d, _ = cKDTree(x).query(x, k=4, workers=16)
    return (d[:, 1:] ** 2).mean(axis=1)


def _knn(pts):
    from simple_knn._C import distCUDA2
    out = distCUDA2(torch.from_numpy(pts).cuda())
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy()


def _check(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.isfinite(got).all()
    zero = want == 0
    np.testing.assert_array_equal(got[zero], 0.0)
    rel = np.abs(got[~zero].astype(np.float64) - want[~zero]) / want[~zero]
    assert rel.size == 0 or rel.max() <= 1e-6, (rel.max(), int(rel.argmax()))


def _cloud(kind, P, seed):
    rs = np.random.RandomState(seed)
    if kind == "uniform":
        x = rs.uniform(-1.0, 1.0, (P, 3))
    elif kind == "nerf":              # the NeRF-synthetic start: uniform in [-1.3, 1.3]^3 (scene/dataset_readers.py of the reference)
        x = rs.random_sample((P, 3)) * 2.6 - 1.3
    elif kind == "clusters":          # tight Gaussian clusters plus 1 % far outliers
        n_out = max(1, P // 100)
        centres = rs.uniform(-5.0, 5.0, (max(1, P // 5000), 3))
        x = centres[rs.randint(0, len(centres), P - n_out)] + 0.01 * rs.randn(P - n_out, 3)
        x = np.concatenate([x, rs.uniform(-500.0, 500.0, (n_out, 3))])
        x = x[rs.permutation(P)]
    elif kind == "plane":             # zero extent along z
        x = np.concatenate([rs.uniform(-2.0, 2.0, (P, 2)), np.full((P, 1), 0.75)], axis=1)
    elif kind == "offset":            # around 1e4 with unit spread: coarse float32 coordinates
        x = 1.0e4 + rs.uniform(-1.0, 1.0, (P, 3))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


SMALL = [4, 5, 63, 64, 65, 4095, 4096, 4097, 262_143]


@pytest.mark.parametrize("P", SMALL + [1_000_000, 5_000_000])
def test_uniform_matches_exact_oracle(P):
    pts = _cloud("uniform", P, P)
    _check(_knn(pts), _oracle(pts))


def test_nerf_synthetic_start_matches_exact_oracle():
    pts = _cloud("nerf", 100_000, 7)
    _check(_knn(pts), _oracle(pts))


@pytest.mark.parametrize("P", [65, 4097, 262_143, 1_000_000])
def test_clusters_with_outliers_match_exact_oracle(P):
    pts = _cloud("clusters", P, 11 + P)
    _check(_knn(pts), _oracle(pts))


@pytest.mark.parametrize("kind", ["plane", "offset"])
@pytest.mark.parametrize("P", [63, 4096, 262_143])
def test_degenerate_clouds_match_exact_oracle(kind, P):
    pts = _cloud(kind, P, 3 + P)
    _check(_knn(pts), _oracle(pts))


def test_fewer_than_four_points():
    from simple_knn._C import distCUDA2
    e = distCUDA2(torch.zeros(0, 3, device="cuda"))
    assert e.shape == (0,) and e.dtype == torch.float32 and e.is_cuda
    for P in (1, 2):
        assert np.isposinf(_knn(np.random.RandomState(P).rand(P, 3).astype(np.float32))).all()
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]], np.float32)
    got = _knn(pts)
    for i in range(3):
        d = np.sort([np.float32(((pts[j] - pts[i]) ** 2).sum()) for j in range(3) if j != i]).astype(np.float32)
        want = np.float32(np.float32(np.float32(d[0] + d[1]) + FLT_MAX) / np.float32(3.0))
        assert got[i] == want and np.isfinite(got[i]), (i, got[i], want)


def test_duplicates_are_neighbours_at_zero():
    """A copy is excluded by index, not by distance: each copy of a pair has the other as a neighbour at 0 (and the two share their other
    neighbours, so their results are equal); four copies of one point leave each of them three neighbours at 0."""
    pts = _cloud("uniform", 10_000, 6)
    pts[100] = pts[9000]
    got, want = _knn(pts), _oracle(pts)
    _check(got, want)
    from scipy.spatial import cKDTree
    assert cKDTree(pts.astype(np.float64)).query(pts[100].astype(np.float64), k=2)[0][1] == 0.0
    assert got[100] == got[9000] > 0.0
    pts[10] = pts[11] = pts[12] = pts[4000]
    got = _knn(pts)
    assert (got[[10, 11, 12, 4000]] == 0.0).all()
    _check(got, _oracle(pts))
    same = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (4096, 1))
    assert (_knn(same) == 0.0).all()


def test_sort_drivers_agree_bit_for_bit():
    import _gsr
    pts = _cloud("clusters", 1_000_000, 21)
    try:
        _gsr.set_option("sort_driver", 0)
        a = _knn(pts)
        _gsr.set_option("sort_driver", 1)
        b = _knn(pts)
    finally:
        _gsr.set_option("sort_driver", 1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_repeatable_and_permutation_invariant_bit_for_bit():
    pts = _cloud("nerf", 300_000, 31)
    a, b = _knn(pts), _knn(pts)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    perm = np.random.RandomState(32).permutation(len(pts))
    c = _knn(np.ascontiguousarray(pts[perm]))
    assert np.array_equal(c.view(np.uint32), a[perm].view(np.uint32))


def test_runs_on_the_current_stream():
    """On a side stream, with the result read after that stream's synchronisation only: the call is ordered behind the upload on the
    same stream, and nothing in it waits on the default stream."""
    from simple_knn._C import distCUDA2
    pts = _cloud("uniform", 500_000, 41)
    want = _oracle(pts)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.from_numpy(pts).pin_memory().cuda(non_blocking=True)
        out = distCUDA2(x)
        host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    _check(host.numpy(), want)
    # non-contiguous input is made contiguous
    wide = torch.from_numpy(np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], axis=1)).cuda()
    _check(distCUDA2(wide[:, :3]).cpu().numpy(), want)


def test_init_from_point_cloud_and_render():
    import math
    from gaussian_renderer import render
    from gsr_init import SH_C0, init_from_point_cloud
    from gsr_train import GaussianTrainState
    from cubemapencoder import CubemapEncoder
    from helpers import S
    rs = np.random.RandomState(51)
    P = 20_000
    pts = np.concatenate([rs.uniform(-1.5, 1.5, (P, 1)), rs.uniform(-1.0, 1.0, (P, 1)), rs.uniform(4.0, 6.0, (P, 1))], axis=1).astype(np.float32)
    rgb = rs.rand(P, 3).astype(np.float32)
    g = torch.Generator(device="cuda").manual_seed(5)
    t = init_from_point_cloud(pts, rgb, sh_degree=3, init_opacity=0.1, init_refl=1e-3, cubemap_resolution=16, generator=g)
    assert set(t) == set(GaussianTrainState.ORDER)
    want_scale = np.sqrt(np.maximum(_oracle(pts), 1e-7)).astype(np.float32)
    sc = t["scales"].cpu().numpy()
    assert sc.shape == (P, 2) and (sc[:, 0] == sc[:, 1]).all()
    np.testing.assert_allclose(sc[:, 0], want_scale, rtol=1e-6)
    shs = t["shs"].cpu().numpy()
    assert shs.shape == (P, 16, 3)
    np.testing.assert_allclose(shs[:, 0, :], (rgb.astype(np.float64) - 0.5) / SH_C0, rtol=1e-6, atol=1e-7)
    assert (shs[:, 1:, :] == 0).all()
    assert (t["opacities"].cpu().numpy() == np.float32(0.1)).all() and t["opacities"].shape == (P, 1)
    assert (t["refl_strengths"].cpu().numpy() == np.float32(1e-3)).all() and t["refl_strengths"].shape == (P, 1)
    rot = t["rotations"].cpu().numpy()
    np.testing.assert_allclose(np.linalg.norm(rot, axis=1), 1.0, rtol=1e-6)
    assert t["cubemap"].shape == (6, 3, 16, 16) and (t["cubemap"].abs() <= 0.5).all() and (t["fail"] == 0).all()
    assert torch.equal(t["means3D"].cpu(), torch.from_numpy(pts))

    st = GaussianTrainState(t, "cuda")
    W, H = 256, 160
    cam = S.make_camera(W, H)
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}

    class View:
        FoVx, FoVy, image_width, image_height = cam["FoVx"], cam["FoVy"], W, H
        world_view_transform, full_proj_transform, camera_center = ct["viewmatrix"], ct["projmatrix"], ct["campos"]
        HWK, R, T, znear, zfar = (H, W, cam["K"]), ct["R"], ct["T"], cam["znear"], cam["zfar"]

    class Pipe:
        depth_ratio, compute_cov3D_python = 0.0, False
    env = CubemapEncoder(output_dim=3, resolution=16).cuda()
    with torch.no_grad():
        env.params["Cubemap_texture"].copy_(st.p["cubemap"])
        env.params["Cubemap_failv"].copy_(st.p["fail"])

    class PC:
        get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (st.p["means3D"], st.p["opacities"], st.p["scales"],
                                                                                   st.p["rotations"], st.p["shs"], st.p["refl_strengths"])
        active_sh_degree, get_envmap = 3, env
    out = render(View, PC, Pipe, torch.zeros(3, device="cuda"))
    img = out["render"]
    assert img.shape == (3, H, W) and torch.isfinite(img).all()
    assert int((out["radii"] > 0).sum()) > P // 2          # the cloud is in front of the camera: most surfels are drawn
    assert math.isfinite(float(img.sum())) and float(img.abs().sum()) > 0
