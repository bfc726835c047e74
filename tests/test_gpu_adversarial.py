"""GPU: the tile kernels on the scene families of tests/adversarial_scenes.py (surfaces seen obliquely, grazing and edge-on splats, values
on every threshold of the blend, exact duplicates), held to the bars of tests/test_gpu_parity.py unchanged:
  * against the oracle: integer state bit-exact, n_contrib within its budget, images within assert_image_close, every gradient within
    rel_maxnorm <= 1e-4 and grad_gate <= GATE_BUDGET (variant G: where the GPU misses those bars, the float32 oracle misses float64 by
    more on these scenes, and the GPU is held to float64 instead, see check_gauss);
  * per-wave culling off against on: every forward output, n_contrib and final_T bit-identical, gradients within 5e-5
    (test_cull_is_bit_exact's bar);
  * the inference forward bit-identical to the training forward (variant S);
and the binning at the sort's block edges: instance counts set exactly (one tiny splat per instance, no near-plane culls) on and around
the depth sort's 4096-item and the tile sort's 16384-item blocks, one tile holding every instance, and tied depth keys, against the oracle
and with both sort drivers.  tests/test_adversarial_reach.py proves on the CPU that each family reaches its target."""
import numpy as np
import pytest

import adversarial_scenes as A
from helpers import GATE_BUDGET, HipGauss, HipSurfel, S, assert_image_close, assert_planes_psnr, grad_gate, n_contrib_ok, psnr, rel_maxnorm

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4
PSNR_MIN = 50.0
S_GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_drefl_strengths", "dL_dscales", "dL_drotations")
G_GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dnormals", "dL_drefl_strengths", "dL_dscales", "dL_drotations")


def _orc():
    from oracle import oracle as orc
    return orc


def check_binning(hip, o):
    """Integer / index state of the binning bit for bit (test_gpu_parity._check_binning)."""
    np.testing.assert_array_equal(hip.state("tiles_touched").astype(np.uint32), o.state("tiles_touched"))
    np.testing.assert_array_equal(hip.state("point_offsets").astype(np.uint32), o.state("point_offsets"))
    vis = o.state("radii") > 0
    np.testing.assert_array_equal(hip.state("depths").view(np.uint32)[vis], o.state("depths").view(np.uint32)[vis])
    np.testing.assert_array_equal(hip.state("keys").astype(np.uint64), o.state("keys"))
    np.testing.assert_array_equal(hip.state("point_list").astype(np.uint32), o.state("point_list"))
    np.testing.assert_array_equal(hip.state("ranges").astype(np.uint32), o.state("ranges"))


def _check_grads(gh, gr, keys):
    for k in keys:
        err = rel_maxnorm(gh[k].reshape(gr[k].shape), gr[k])
        assert err <= GRAD_TOL, (k, err)
        bad = grad_gate(gh[k], gr[k], GRAD_TOL)
        assert bad <= GATE_BUDGET, (k, "elementwise gate", bad)


def check_surfel(kw, seed, backward=True):
    """Variant S against the oracle with the checks of test_gpu_parity._run_surfel."""
    H, W = kw["image_height"], kw["image_width"]
    o = _orc().SurfelOracle(np.float32)
    ref = o.forward(**kw)
    hip = HipSurfel(kw)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"]
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    check_binning(hip, o)
    nc_h, nc_o = hip.state("n_contrib").astype(np.uint32), o.state("n_contrib")
    assert n_contrib_ok(nc_h[0], nc_o[0]) and n_contrib_ok(nc_h[1], nc_o[1])
    assert psnr(out["color"], ref["color"]) >= PSNR_MIN
    assert_image_close(out["color"], ref["color"], 3e-5)
    assert psnr(out["refl_strength_map"], ref["refl_strength_map"]) >= PSNR_MIN
    assert_planes_psnr(out["allmap"], ref["allmap"])
    gw_h, gw_o = out["gaussian_weights"].astype(np.float64), ref["gaussian_weights"].astype(np.float64)
    gw_bad = np.abs(gw_h - gw_o) > 1.5e-6 + 1e-5 * np.abs(gw_o)
    assert int(gw_bad.sum()) <= max(2, int(3e-5 * gw_o.size)) and np.abs(gw_h - gw_o).max() <= 5e-3, (int(gw_bad.sum()), np.abs(gw_h - gw_o).max())
    if not backward:
        return
    g = S.make_upstream_grads(H, W, seed)
    gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dallmap=g["dL_dplanes"], dL_drefl_strength_map=g["dL_drefl"])
    gh = hip.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"])
    keys = S_GRADS if kw.get("cov3D_precomp") is None else S_GRADS[:5] + ("dL_dtransMat",)
    _check_grads(gh, gr, keys)


def check_gauss(kw, seed, antialiasing, backward=True):
    """Variant G against the oracle with the checks of test_gpu_parity._run_gauss."""
    H, W = kw["image_height"], kw["image_width"]
    o = _orc().GaussOracle(np.float32)
    ref = o.forward(antialiasing=antialiasing, **kw)
    hip = HipGauss(kw, antialiasing=antialiasing)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"]
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    check_binning(hip, o)
    assert n_contrib_ok(hip.state("n_contrib").astype(np.uint32)[0], o.state("n_contrib"))
    for k in ("color", "normal_map", "refl_strength_map", "invdepth"):
        assert psnr(out[k], ref[k], peak=max(1.0, float(np.abs(ref[k]).max()))) >= PSNR_MIN, k
    assert_image_close(out["color"], ref["color"], 5e-4)
    if not backward:
        return
    g = S.make_upstream_grads(H, W, seed)
    gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dinvdepth=g["dL_dinvdepth"], dL_dnormal_map=g["dL_dnormal"], dL_drefl_strength_map=g["dL_drefl"])
    gh = hip.backward(g["dL_dcolor"], g["dL_dinvdepth"], g["dL_dnormal"], g["dL_drefl"])
    gr64 = None
    for k in G_GRADS:
        err = rel_maxnorm(gh[k].reshape(gr[k].shape), gr[k])
        bad = grad_gate(gh[k], gr[k], GRAD_TOL)
        if err <= GRAD_TOL and bad <= GATE_BUDGET:
            continue
        # These scenes put the variant-G gradients past fp32 resolution: the float32 oracle itself misses the float64 one by up to 1e-3
        # in max-norm (scales, rotations and means of flat, oblique 3D Gaussians) and on 0.02 - 6 % of the elements of every gradient
        # (sums over many pixels that cancel).  There the GPU is held to float64: no further from it than the float32 restatement
        # (twice its distance, plus the bar)
        if gr64 is None:
            o64 = _orc().GaussOracle(np.float64)
            o64.forward(antialiasing=antialiasing, **kw)
            gr64 = o64.backward(dL_dcolor=g["dL_dcolor"], dL_dinvdepth=g["dL_dinvdepth"], dL_dnormal_map=g["dL_dnormal"], dL_drefl_strength_map=g["dL_drefl"])
        err64, orc_err64 = rel_maxnorm(gh[k].reshape(gr64[k].shape), gr64[k]), rel_maxnorm(gr[k], gr64[k])
        assert err64 <= 2 * orc_err64 + GRAD_TOL, (k, "max-norm against float64", err, err64, orc_err64)
        bad64, orc_bad64 = grad_gate(gh[k], gr64[k], GRAD_TOL), grad_gate(gr[k], gr64[k], GRAD_TOL)
        # (plus two elements, the floor of n_contrib_ok and assert_image_close: a pair whose alpha or T sits within an ulp of a threshold
        # blends on one side and not on the other and moves its Gaussian's gradient by its whole share)
        assert bad64 * gh[k].size <= 2 * orc_bad64 * gh[k].size + max(2, GATE_BUDGET * gh[k].size), (k, "elementwise gate against float64",
                                                                                                         bad, bad64, orc_bad64)


def _run_hip(variant, kw, antialiasing, g):
    if variant == "S":
        hip = HipSurfel(kw)
        out, nc, ft = hip.out(), hip.state("n_contrib"), hip.state("final_T")
        gh = hip.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"])
    else:
        hip = HipGauss(kw, antialiasing=antialiasing)
        out, nc, ft = hip.out(), hip.state("n_contrib"), hip.state("final_T")
        gh = hip.backward(g["dL_dcolor"], g["dL_dinvdepth"], g["dL_dnormal"], g["dL_drefl"])
    return out, gh, nc, ft


def check_cull_bit_identity(variant, kw, seed, antialiasing=False):
    """Culling only skips pairs that cannot blend: outputs, n_contrib and final_T the same bits with the vote off and on."""
    import _gsr
    g = S.make_upstream_grads(kw["image_height"], kw["image_width"], seed)
    res = []
    try:
        for cull in (0, 1):
            _gsr.set_option("cull", cull)
            res.append(_run_hip(variant, kw, antialiasing, g))
    finally:
        _gsr.set_option("cull", 1)
    (o0, g0, n0, t0), (o1, g1, n1, t1) = res
    for k in o0:
        if isinstance(o0[k], np.ndarray):
            np.testing.assert_array_equal(o0[k], o1[k], err_msg=k)
        else:
            assert o0[k] == o1[k], k
    np.testing.assert_array_equal(n0, n1)
    np.testing.assert_array_equal(t0, t1)
    bar = {k: 5e-5 for k in g0}
    if variant == "G":
        # (see check_gauss) two runs that differ only in the order of the float atomics: held to 5e-5, or to the float32 oracle's own
        # distance from float64, twice over, where that is larger (scales, rotations and means of flat 3D Gaussians)
        gr = []
        for dt in (np.float32, np.float64):
            o = _orc().GaussOracle(dt)
            o.forward(antialiasing=antialiasing, **kw)
            gr.append(o.backward(dL_dcolor=g["dL_dcolor"], dL_dinvdepth=g["dL_dinvdepth"], dL_dnormal_map=g["dL_dnormal"], dL_drefl_strength_map=g["dL_drefl"]))
        for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations"):
            bar[k] = max(5e-5, 2 * rel_maxnorm(gr[0][k], gr[1][k]))
    for k in g0:
        if g0[k] is not None:
            assert rel_maxnorm(g1[k], g0[k]) <= bar[k], (k, rel_maxnorm(g1[k], g0[k]), bar[k])


CASES = [("S", None), ("G", True), ("G", False)]
FAMILIES = ["surface", "grazing", "threshold", "dup_surface", "dup_threshold"]


def _case_id(c):
    return c[0] if c[1] is None else c[0] + ("_aa" if c[1] else "_noaa")


def _kw(name, variant):
    P, W, H, seed = A.SCENES[name]
    return A.family(name, variant, P, W, H, seed), seed


@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("name", FAMILIES)
def test_family_against_oracle(name, case):
    variant, aa = case
    kw, seed = _kw(name, variant)
    if variant == "S":
        check_surfel(kw, seed)
    else:
        check_gauss(kw, seed, aa)


def test_degenerate_homographies_against_oracle():
    """Precomputed homographies, every third with the camera centre in its plane (p.z == 0 at every pixel): the grazing branches of the
    forward and the backward on every lane, gradients to the homography itself."""
    kw, seed = _kw("grazing_T", "S")
    check_surfel(kw, seed)


@pytest.mark.parametrize("name,case", [(n, c) for n in FAMILIES for c in CASES] + [("grazing_T", CASES[0])],
                         ids=lambda x: x if isinstance(x, str) else _case_id(x))
def test_family_cull_bit_identity(name, case):
    variant, aa = case
    kw, seed = _kw(name, variant)
    check_cull_bit_identity(variant, kw, seed, aa)


def check_eval_forward(kw):
    """gsr_surfel_forward_eval against the training forward on the outputs they share: the same bits."""
    import torch
    from diff_surfel_rasterization import _C
    from helpers import to_cuda
    t = to_cuda(kw)
    e = torch.empty(0, device="cuda")
    o = lambda k: e if t.get(k) is None else t[k]
    a = [t["bg"], t["means3D"], e, t["refl_strengths"], t["opacities"], o("scales"), o("rotations"), 1.0, o("cov3D_precomp"), t["viewmatrix"],
         t["projmatrix"], kw["tanfovx"], kw["tanfovy"], kw["image_height"], kw["image_width"], t["shs"], kw["sh_degree"], t["campos"], False, False]
    tr = _C.rasterize_gaussians(*a[:2], t["env_scope_mask"], *a[2:], refl=None)
    ev = _C.rasterize_gaussians_eval(*a, refl=None)
    torch.cuda.synchronize()
    n_tr, color, others, radii, refl_map = tr[0], tr[1], tr[2], tr[3], tr[7]
    n_ev, e_color, e_alpha, e_normal, e_refl_map, e_radii = ev[:6]
    assert n_ev == n_tr > 0
    assert torch.equal(e_radii, radii)
    assert torch.equal(e_color, color)
    assert torch.equal(e_alpha, others[1:2])
    assert torch.equal(e_normal, others[2:5])
    assert torch.equal(e_refl_map, refl_map)


@pytest.mark.parametrize("name", FAMILIES + ["grazing_T"])
def test_family_eval_forward_is_bit_identical(name):
    check_eval_forward(_kw(name, "S")[0])


# ------------------------------------------------------------------------------------------- full size
def test_surface_family_at_c3_size():
    """The surface family at the C3 size (10^6 surfels, 1920x1080, SH 3): the checks of test_gpu_fullsize.test_c3_against_oracle, and
    culling off against on."""
    import _gsr
    P, W, H = 1_000_000, 1920, 1080
    kw, cam = A.surface("S", P, W, H, 1003)
    o = _orc().SurfelOracle(np.float32)
    ref = o.forward(**kw)
    hip = HipSurfel(kw)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"] > P
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    np.testing.assert_array_equal(hip.state("point_list").astype(np.uint32), o.state("point_list"))
    assert n_contrib_ok(hip.state("n_contrib"), o.state("n_contrib"))
    assert psnr(out["color"], ref["color"]) >= 50
    assert_planes_psnr(out["allmap"], ref["allmap"])
    g = S.make_upstream_grads(H, W, 1003)
    gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dallmap=g["dL_dplanes"], dL_drefl_strength_map=g["dL_drefl"])
    gh = hip.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"])
    _check_grads(gh, gr, S_GRADS)
    del o, ref, gr, gh, hip
    outs = []
    try:
        for cull in (1, 0):
            _gsr.set_option("cull", cull)
            hip = HipSurfel(kw)
            outs.append((hip.out(), hip.state("n_contrib"), hip.state("final_T")))
            del hip
    finally:
        _gsr.set_option("cull", 1)
    (a, na, ta), (b, nb, tb) = outs
    for k in ("color", "allmap", "refl_strength_map", "gaussian_weights", "radii"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(na, nb) and np.array_equal(ta, tb)


# ------------------------------------------------------------------------------------------- sort block edges and ties
def exact_instances(variant, P, W, H, seed, one_tile=False, dup=False):
    """P tiny splats (footprint radius 3 px) at tile centres, depths 2..6: each touches exactly one tile and none is culled, so
    num_rendered == P.  one_tile: all in the tile at the image centre (every tile key equal).  dup: the second half copies the first
    (tied depth keys, ordered by Gaussian index)."""
    rs = np.random.RandomState(seed)
    cam = S.make_camera(W, H)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    if one_tile:
        tx, ty = np.full(P, gx // 2), np.full(P, gy // 2)
    else:
        t = rs.randint(0, gx * gy, P)
        tx, ty = t % gx, t // gx
    z = rs.uniform(2.0, 6.0, P)
    means = A._pixel_to_world(cam, tx * 16 + 7.5, ty * 16 + 7.5, z)
    n = rs.randn(P, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    tang = np.full((P, 2), 1e-4) * z[:, None]
    sc = A._attributes(P, variant, rs, means, A._scales(variant, P, rs, tang), A._rot_for_normal(n, rs), rs.uniform(0.2, 0.9, P), n)
    kw = A._kw(variant, sc, cam, 1, (0.1, 0.2, 0.3))
    kw["shs"] = np.ascontiguousarray(kw["shs"][:, :4])
    return A.duplicates(kw) if dup else kw


def check_exact_binning(variant, kw, P):
    """Binning bit-exact against the oracle, num_rendered == P, and both sort drivers giving the same bits."""
    import _gsr
    o = (_orc().SurfelOracle if variant == "S" else _orc().GaussOracle)(np.float32)
    ref = o.forward(**kw)
    assert ref["num_rendered"] == P
    res = []
    try:
        for driver in (1, 0):
            _gsr.set_option("sort_driver", driver)
            hip = HipSurfel(kw) if variant == "S" else HipGauss(kw)
            out = hip.out()
            assert out["num_rendered"] == P
            np.testing.assert_array_equal(out["radii"], ref["radii"])
            check_binning(hip, o)
            assert n_contrib_ok(hip.state("n_contrib").astype(np.uint32).reshape(o.state("n_contrib").shape), o.state("n_contrib"))
            res.append((out, {k: hip.state(k) for k in ("point_list", "ranges", "keys", "n_contrib")}))
    finally:
        _gsr.set_option("sort_driver", 1)
    (o1, s1), (o0, s0) = res
    for k in s1:
        np.testing.assert_array_equal(s1[k], s0[k], err_msg=k)
    np.testing.assert_array_equal(o1["color"], o0["color"])


@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("P", [4095, 4096, 4097, 8192])
def test_depth_sort_block_edges(variant, P):
    """The depth sort's blocks hold 1024 x 4 items: P one item short of, exactly on, and one past a block boundary."""
    check_exact_binning(variant, exact_instances(variant, P, 328, 232, P), P)


@pytest.mark.parametrize("P", [16383, 16384, 16385])
def test_tile_sort_block_edges(P):
    """The default tile sort's blocks hold 1024 x 16 items."""
    check_exact_binning("S", exact_instances("S", P, 328, 232, P + 1), P)


@pytest.mark.parametrize("variant", ["S", "G"])
def test_every_instance_in_one_tile(variant):
    check_exact_binning(variant, exact_instances(variant, 4097, 200, 136, 77, one_tile=True), 4097)


@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("one_tile", [False, True])
def test_tied_depth_keys_order_by_index(variant, one_tile):
    kw = exact_instances(variant, 8192, 328, 232, 78, one_tile=one_tile, dup=True)
    check_exact_binning(variant, kw, 8192)
