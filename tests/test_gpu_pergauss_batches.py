"""Variant S's per-Gaussian forward walks the scene in batches of 256, a fixed grid of workgroups making several trips, and every lane fetches
its next surfel's inputs while it computes the current one (pergauss_batches, csrc/gsr_internal.hpp).  What can go wrong lies at the batch
edges: a lane that prefetches past P, a ragged last batch, a grid larger than the work, a trip whose whole batch is culled.  The backward
reads the SH row only where the colour gradient is non-zero; both extremes are here too.  Everything is compared with the CPU oracle on a
40x24 image at SH degree 3, forward and backward, with the helpers and the bars of tests/test_gpu_parity.py; the surfels of the large scenes
are small (mu = -6) so that they stay cheap for the tile kernels.

Variant S runs at every size.  Its backward pass and both passes of variant G are one-shot kernels (one workgroup per batch: "pergauss_grid"
reports no resident slots for them), so the sizes derived from the grid are the forward's; variant G runs the fixed sizes."""
import numpy as np
import pytest
import torch

from helpers import GATE_BUDGET, HipGauss, HipSurfel, S, assert_image_close, grad_gate, n_contrib_ok, psnr, rel_maxnorm, scene_kwargs
from test_gpu_parity import GRAD_TOL, PSNR_MIN, _check_binning

pytestmark = pytest.mark.gpu

W, H = 40, 24
MU = -6.0
S_GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_drefl_strengths", "dL_dscales", "dL_drotations")
G_GRADS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dnormals", "dL_drefl_strengths", "dL_dscales", "dL_drotations")


def _oracle():
    from oracle import oracle as orc
    return orc


def _grid(variant, P):
    """(forward grid, backward grid, forward slots, backward slots) of the per-Gaussian passes for P Gaussians, from the library."""
    import _gsr
    dummy = torch.zeros(4, dtype=torch.int32, device="cuda")
    return [int(x) for x in _gsr.debug_fetch(variant, "pergauss_grid", P, 0, W, H, dummy, dummy, dummy, torch.int32, (4,)).cpu().numpy()]


def _gate(gh, gr, names):
    for k in names:
        err = rel_maxnorm(gh[k].reshape(gr[k].shape), gr[k])
        assert err <= GRAD_TOL, (k, err)
        bad = grad_gate(gh[k], gr[k], GRAD_TOL)
        assert bad <= GATE_BUDGET, (k, "elementwise gate", bad)


def _check_surfel(kw, seed, grads=None, make_hip=HipSurfel):
    """tests/test_gpu_parity.py::_run_surfel from the scene on; `grads`: the upstream gradients (default: S.make_upstream_grads)."""
    o = _oracle().SurfelOracle(np.float32)
    ref = o.forward(**kw)
    hip = make_hip(kw)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"]
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    _check_binning(hip, o)
    nc_h, nc_o = hip.state("n_contrib").astype(np.uint32), o.state("n_contrib")
    assert n_contrib_ok(nc_h[0], nc_o[0]) and n_contrib_ok(nc_h[1], nc_o[1])
    assert psnr(out["color"], ref["color"]) >= PSNR_MIN
    assert_image_close(out["color"], ref["color"], 3e-5)
    assert psnr(out["refl_strength_map"], ref["refl_strength_map"]) >= PSNR_MIN
    for plane in range(8):
        scale = max(1.0, float(np.abs(ref["allmap"][plane]).max()))
        assert psnr(out["allmap"][plane], ref["allmap"][plane], peak=scale) >= PSNR_MIN, plane
    gw_h, gw_o = out["gaussian_weights"].astype(np.float64), ref["gaussian_weights"].astype(np.float64)
    gw_bad = np.abs(gw_h - gw_o) > 1.5e-6 + 1e-5 * np.abs(gw_o)
    assert int(gw_bad.sum()) <= max(2, int(3e-5 * gw_o.size)) and np.abs(gw_h - gw_o).max() <= 5e-3, (int(gw_bad.sum()), np.abs(gw_h - gw_o).max())
    g = grads or S.make_upstream_grads(H, W, seed)
    gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dallmap=g["dL_dplanes"], dL_drefl_strength_map=g["dL_drefl"])
    gh = hip.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"])
    _gate(gh, gr, S_GRADS)
    return hip, ref, gh, gr


def _check_gauss(kw, seed):
    """tests/test_gpu_parity.py::_run_gauss from the scene on."""
    o = _oracle().GaussOracle(np.float32)
    ref = o.forward(antialiasing=True, **kw)
    hip = HipGauss(kw, antialiasing=True)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"]
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    _check_binning(hip, o)
    assert n_contrib_ok(hip.state("n_contrib").astype(np.uint32)[0], o.state("n_contrib"))
    for k in ("color", "normal_map", "refl_strength_map", "invdepth"):
        scale = max(1.0, float(np.abs(ref[k]).max()))
        assert psnr(out[k], ref[k], peak=scale) >= PSNR_MIN, k
    assert_image_close(out["color"], ref["color"], 5e-4)
    g = S.make_upstream_grads(H, W, seed)
    gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dinvdepth=g["dL_dinvdepth"], dL_dnormal_map=g["dL_dnormal"], dL_drefl_strength_map=g["dL_drefl"])
    gh = hip.backward(g["dL_dcolor"], g["dL_dinvdepth"], g["dL_dnormal"], g["dL_drefl"])
    _gate(gh, gr, G_GRADS)


# ---- sizes about a wave and about one batch: one workgroup, or two with a one-row second batch
@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_about_a_wave_and_a_batch(variant, P):
    kw, _, _ = scene_kwargs(variant, P, W, H, 300 + P, -2.0, 3, (0.2, 0.1, 0.3), mask_radius=4.5 if variant == "S" else 0.0)
    if variant == "S":
        _check_surfel(kw, 300 + P)
    else:
        _check_gauss(kw, 300 + P)


# ---- sizes about the grid: G x 256 - 1, G x 256 and G x 256 + 1 with G the resident slots of the forward pass (one trip that fills the grid
# exactly, then a second trip of one row), and 3 x G x 256 + 65 (several trips, a ragged last one)
@pytest.mark.parametrize("mult,add", [(1, -1), (1, 0), (1, 1), (3, 65)])
def test_sizes_about_the_grid(mult, add):
    slots = _grid(0, 1)[2]
    assert slots > 0
    P = mult * slots * 256 + add
    launched, bwd = _grid(0, P)[:2]
    nb = (P + 255) // 256
    assert bwd == nb                                      # the backward: one workgroup per batch
    assert 0 < launched <= min(slots, nb)
    trips = -(-nb // launched)
    assert trips == -(-nb // slots)                     # no more trips than the full grid would make
    assert trips == (1 if add <= 0 else mult + 1)        # the sizes do what their names say
    kw, _, _ = scene_kwargs("S", P, W, H, 17 * mult + add, MU, 3, (0.0, 0.0, 0.0), mask_radius=4.5)
    _check_surfel(kw, 5)


# ---- every surfel of one whole batch behind the camera: first, in the middle, last
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_whole_batch_culled(where):
    P = 5 * 256 + 77
    kw, cam, _ = scene_kwargs("S", P, W, H, 41, -2.5, 3, (0.1, 0.2, 0.0), mask_radius=4.5)
    nb = (P + 255) // 256
    b = {"first": 0, "middle": nb // 2, "last": nb - 1}[where]
    lo, hi = b * 256, min(P, b * 256 + 256)
    # behind the camera: reflect the batch through the camera position along the viewing direction (view-space z -> -z)
    vm = np.asarray(cam["viewmatrix"], np.float64).reshape(4, 4)     # row-vector convention: p_view = [p, 1] @ vm
    m = kw["means3D"].astype(np.float64).copy()
    z = m[lo:hi] @ vm[:3, 2] + vm[3, 2]
    axis = vm[:3, 2] / np.dot(vm[:3, 2], vm[:3, 2])
    m[lo:hi] -= np.outer(z + np.abs(z) + 1.0, axis)                   # z -> -|z| - 1
    kw["means3D"] = m.astype(np.float32)
    hip, ref, _, _ = _check_surfel(kw, 41)
    assert (ref["radii"][lo:hi] == 0).all() and (ref["radii"] > 0).any()


# ---- accumulate mode: two views into one sink against the sum of two overwrite-mode runs
def test_backward_accumulates_two_views():
    from gsr_dist import FlatGrads
    P = 3 * 256 + 65
    names = dict(means3D="dL_dmeans3D", shs="dL_dsh", opacities="dL_dopacity", scales="dL_dscales", rotations="dL_drotations",
                 refl_strengths="dL_drefl_strengths")
    params = lambda h: dict(means3D=h.means3D, shs=h.shs, opacities=h.opac, scales=h.scales, rotations=h.rots, refl_strengths=h.refl)
    kwa, _, _ = scene_kwargs("S", P, W, H, 91, -2.5, 3, (0.1, 0.0, 0.2), mask_radius=4.5)
    kwb = dict(kwa)
    camb = S.look_at_camera(W, H, eye=(0.5, -0.2, -0.4))
    for k in ("viewmatrix", "projmatrix", "campos"):
        kwb[k] = camb[k]
    g = S.make_upstream_grads(H, W, 8)
    bwd = lambda h: h.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"])
    ga, gb = bwd(HipSurfel(kwa)), bwd(HipSurfel(kwb))
    box = {}

    def sink(acc):
        def f(h):
            if "fg" not in box:
                box["fg"] = FlatGrads(params(h))
                box["fg"].flat.fill_(float("nan"))
            return box["fg"].sink(), acc
        return f
    bwd(HipSurfel(kwa, make_sink=sink(False)))
    fg = box["fg"]
    for k, name in names.items():
        got = fg.view(k).cpu().numpy()
        assert np.isfinite(got).all(), k                                   # every element was written
        assert rel_maxnorm(got, ga[name].reshape(got.shape)) <= 5e-5, k    # (the float atomics of the tile backward order differently)
    bwd(HipSurfel(kwb, make_sink=sink(True)))
    for k, name in names.items():
        got = fg.view(k).cpu().numpy()
        assert rel_maxnorm(got, (ga[name] + gb[name]).reshape(got.shape)) <= 5e-5, k
        assert rel_maxnorm(got, gb[name].reshape(got.shape)) > 1e-3, k      # really the sum, not the last view


# ---- the backward's conditional SH prefetch: no surfel with a colour gradient, every visible surfel with one
def test_backward_without_any_colour_gradient():
    P = 2 * 256 + 65
    kw, _, _ = scene_kwargs("S", P, W, H, 53, -2.0, 3, (0.0, 0.0, 0.0), mask_radius=4.5)
    g = S.make_upstream_grads(H, W, 53)
    g["dL_dcolor"] = np.zeros_like(g["dL_dcolor"])
    _, _, gh, _ = _check_surfel(kw, 53, grads=g)
    assert not gh["dL_dsh"].any()
    assert np.abs(gh["dL_dmeans3D"]).max() > 0           # the planes' gradients still arrive


def test_backward_with_a_colour_gradient_on_every_surfel():
    P = 2 * 256 + 65
    # large translucent surfels in front of the camera: every one blends into some pixel before the pixels saturate
    kw, _, _ = scene_kwargs("S", P, W, H, 54, -1.5, 3, (0.0, 0.0, 0.0), mask_radius=4.5)
    kw["opacities"] = np.full_like(kw["opacities"], 0.02)
    g = S.make_upstream_grads(H, W, 54)
    g["dL_dcolor"] = np.abs(g["dL_dcolor"]) + 0.5
    _, ref, gh, gr = _check_surfel(kw, 54, grads=g)
    touched = np.abs(gr["dL_dsh"]).reshape(P, -1).sum(axis=1) > 0
    vis = ref["radii"] > 0
    assert vis.sum() > 256 and (touched[vis]).mean() > 0.9, (int(vis.sum()), float(touched[vis].mean()))
    np.testing.assert_array_equal(np.abs(gh["dL_dsh"]).reshape(P, -1).sum(axis=1) > 0, touched)


# ---- the inputs fill their allocation to the last byte: P = 257 rows and no slack behind them.  The prefetch clamps its row to P - 1
# (pergauss_batches), so nothing past row P - 1 is read; here the bytes behind every input are another tensor's, filled with NaN, and the
# outputs must not change
def test_inputs_without_slack_behind_the_last_row():
    P = 257
    kw, _, _ = scene_kwargs("S", P, W, H, 77, -2.0, 3, (0.2, 0.1, 0.3), mask_radius=4.5)

    class Tight(HipSurfel):
        """HipSurfel over inputs that are each the LAST elements of a fresh block (HipSurfel itself clones what it is given)."""

        def __init__(self, kw_):
            from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer

            def last(a, dtype=torch.float32):
                a = torch.from_numpy(np.ascontiguousarray(a))
                n = a.numel()
                block = torch.empty(n + (-n) % 64, dtype=dtype, device="cuda")      # (64 elements: the start stays 16-byte aligned)
                block.fill_(float("nan") if dtype == torch.float32 else 1)
                block[block.numel() - n:] = a.reshape(-1).to(dtype)
                return block[block.numel() - n:].view(a.shape)
            self.P, self.H, self.W = P, H, W
            leaf = lambda k: last(kw_[k]).detach().requires_grad_(True)
            self.means3D, self.opac, self.shs, self.refl = leaf("means3D"), leaf("opacities"), leaf("shs"), leaf("refl_strengths")
            self.scales, self.rots = leaf("scales"), leaf("rotations")
            self.means2D = torch.zeros_like(self.means3D).requires_grad_(True)
            self.colors = self.cov = None
            cu = lambda k: torch.from_numpy(kw_[k]).cuda()
            st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=kw_["tanfovx"], tanfovy=kw_["tanfovy"], bg=cu("bg"),
                                               scale_modifier=1.0, viewmatrix=cu("viewmatrix"), projmatrix=cu("projmatrix"),
                                               sh_degree=kw_["sh_degree"], campos=cu("campos"), prefiltered=False, debug=False)
            self.color, self.radii, self.allmap, self.refl_map, self.gw = GaussianRasterizer(st)(
                means3D=self.means3D, means2D=self.means2D, opacities=self.opac, shs=self.shs, colors_precomp=None, refl_strengths=self.refl,
                scales=self.scales, rotations=self.rots, cov3D_precomp=None, env_scope_mask=last(kw_["env_scope_mask"], torch.bool))
            self.ctx = self.color.grad_fn
            self.R = self.ctx.num_rendered
            for t in (self.means3D, self.opac, self.shs, self.refl, self.scales, self.rots):      # each ends where its block ends
                assert t.data_ptr() + t.numel() * 4 == t.untyped_storage().data_ptr() + t.untyped_storage().nbytes()
    _, _, gh, _ = _check_surfel(kw, 77, make_hip=Tight)
    for k, v in gh.items():
        assert v is None or np.isfinite(v).all(), k
