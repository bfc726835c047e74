"""Known answers for the outputs of the reference that are NOT true gradients, each
derived by hand from the text of the quirk and evaluated with the dense float64 restatement (tests/dense_torch.py), then
compared with what the oracle returns.  Together with test_oracle_dense.py this pins every backward output of the oracle
against something that does not share its derivation.  CPU only."""
import numpy as np
import pytest
import torch

import dense_torch as dn
from cameras import backward_size, hwk_camera, rolled_pose, trunc_search
from oracle import oracle as orc
from test_oracle_dense import H, TAN, W, _assert_close, _camera, _general_camera, _in_view, _scene, _t


def _gauss_oracle(p, view, full, campos, bg):
    o = orc.GaussOracle(np.float64)
    o.forward(bg=bg, means3D=p["means3D"], opacities=p["opacities"], viewmatrix=view, projmatrix=full, campos=campos, tanfovx=TAN, tanfovy=TAN,
              image_height=H, image_width=W, sh_degree=3, shs=p["shs"], normals=p["normals"], refl_strengths=p["refl_strengths"],
              scales=p["scales"], rotations=p["rotations"])
    return o


def test_gauss_mean2d_pixels_is_the_3_2_1_weighted_colour_gradient():
    """DGR backward.cu:603-655: `dL_dalpha_means2d` is accumulated INSIDE the colour-channel loop as a running sum of the
    partial dL_dalpha, so channel c enters with weight 3 - c; normal / reflection / inverse-depth channels do not enter at
    all; the background term enters unweighted; and the result is scaled to NDC units (x 0.5 W, 0.5 H).  Hence
        grad_means2D = (0.5 W, 0.5 H) * d/d(xy) [ sum_c (3 - c) <g_c, C_c without background> + sum_c <g_c, bg_c T_final> ]
    which autograd evaluates on the dense model through a leaf added to the screen-space means."""
    P = 24
    p = _scene("G", P, 7)
    view, full, campos = _camera(7)
    bg = np.array([0.3, 0.1, 0.6])
    o = _gauss_oracle(p, view, full, campos, bg)
    rs = np.random.RandomState(70)
    wc, wn, wr, wi = rs.normal(size=(3, H, W)), rs.normal(size=(3, H, W)), rs.normal(size=(1, H, W)), rs.normal(size=(1, H, W))
    g = o.backward(dL_dcolor=wc, dL_dinvdepth=wi, dL_dnormal_map=wn, dL_drefl_strength_map=wr)
    off = torch.zeros(P, 2, dtype=torch.float64, requires_grad=True)
    t = {k: _t(p[k], False) for k in ("means3D", "scales", "rotations", "opacities", "shs", "normals", "refl_strengths")}
    out = dn.render_gauss(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["normals"], t["refl_strengths"], _t(view, False),
                          _t(full, False), _t(campos, False), TAN, TAN, W, H, _t(bg, False), xy_offset=off)
    k = torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64)[:, None, None]
    quirk_loss = (k * _t(wc, False) * out["color_nobg"]).sum() + (_t(wc, False) * _t(bg, False)[:, None, None] * out["final_T"][None]).sum()
    quirk_loss.backward()
    expect = off.grad.numpy() * np.array([0.5 * W, 0.5 * H])
    got = g["dL_dmeans2D"]
    assert np.abs(expect).max() > 0
    _assert_close(got[:, :2], expect, 1e-8, "dL_dmean2D_pixels")
    assert np.abs(got[:, 2]).max() == 0
    # ... and it is NOT the true screen-space gradient of the loss the other outputs were differentiated for
    off2 = torch.zeros(P, 2, dtype=torch.float64, requires_grad=True)
    out2 = dn.render_gauss(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["normals"], t["refl_strengths"], _t(view, False),
                           _t(full, False), _t(campos, False), TAN, TAN, W, H, _t(bg, False), xy_offset=off2)
    ((out2["color"] * _t(wc, False)).sum() + (out2["normal_map"] * _t(wn, False)).sum() + (out2["refl_strength_map"] * _t(wr, False)).sum() +
     (out2["invdepth"] * _t(wi, False)).sum()).backward()
    true_ndc = off2.grad.numpy() * np.array([0.5 * W, 0.5 * H])
    assert np.abs(true_ndc - got[:, :2]).max() > 1e-3 * np.abs(true_ndc).max()
    # the internal gradient that feeds dL_dmeans3D (Appendix A.2: "dL_dmean2D, full dL_dalpha") IS that true gradient
    _assert_close(g["dL_dmeans2D_internal"][:, :2], true_ndc, 1e-8, "dL_dmean2D (internal)")


def test_gauss_frustum_clamp_holds_the_clamped_coordinate_constant():
    """DGR forward.cu computeCov2D / backward.cu computeCov2DCUDA: beyond 1.3 x the FoV the view-space x (y) that enters the projection
    Jacobian is replaced by lim * t.z; the backward zeroes its dL/dt.x there but keeps the unclamped formula 2 fx t.x / t.z^3 for
    dL/dt.z, i.e. differentiates J with the clamped coordinate held constant (dense_torch.render_gauss, reference_clamp_gradient).
    A scene with large Gaussians beyond the limit in x, in y and in both, under an anisotropic, off-centre, rolled camera: with the
    option the oracle agrees on every row; without it (plain autograd of the forward) exactly the clamped rows of dL_dmeans3D differ."""
    P = 48
    cam = _general_camera("all", 3)
    view, full, campos, tanx, tany, w, h = cam
    p = _scene("G", P, 13, log_scale=-0.9)
    rs = np.random.RandomState(130)
    pv = p["means3D"] * np.array([tanx / TAN, tany / TAN, 1.0])
    k = np.arange(8, 32)                                   # 8 beyond the limit in x, 8 in y, 8 in both; their 3-sigma extent reaches the image
    beyond = rs.uniform(1.35, 1.6, (len(k), 2)) * rs.choice([-1.0, 1.0], (len(k), 2))
    inside = rs.uniform(-0.9, 0.9, (len(k), 2))
    ndc = np.where(np.stack([(k - 8) // 8 != 1, (k - 8) // 8 != 0], 1), beyond, inside)
    pv[k, 0], pv[k, 1] = ndc[:, 0] * tanx * pv[k, 2], ndc[:, 1] * tany * pv[k, 2]
    p["means3D"] = (pv - view[3, :3]) @ np.linalg.inv(view[:3, :3])
    p["scales"][k] *= 2.5
    bg = np.array([0.3, 0.1, 0.6])
    o = orc.GaussOracle(np.float64)
    ref = o.forward(bg=bg, means3D=p["means3D"], opacities=p["opacities"], viewmatrix=view, projmatrix=full, campos=campos, tanfovx=tanx,
                    tanfovy=tany, image_height=h, image_width=w, sh_degree=3, shs=p["shs"], normals=p["normals"],
                    refl_strengths=p["refl_strengths"], scales=p["scales"], rotations=p["rotations"])
    rs = np.random.RandomState(73)
    wc, wn, wr, wi = rs.normal(size=(3, h, w)), rs.normal(size=(3, h, w)), rs.normal(size=(1, h, w)), rs.normal(size=(1, h, w))
    g = o.backward(dL_dcolor=wc, dL_dinvdepth=wi, dL_dnormal_map=wn, dL_drefl_strength_map=wr)
    res = {}
    for option in (True, False):
        t = {k_: _t(p[k_]) for k_ in ("means3D", "scales", "rotations", "opacities", "shs", "normals", "refl_strengths")}
        out = dn.render_gauss(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["normals"], t["refl_strengths"],
                              _t(view, False), _t(full, False), _t(campos, False), tanx, tany, w, h, _t(bg, False),
                              reference_clamp_gradient=option)
        np.testing.assert_array_equal(out["radii"].numpy(), ref["radii"])
        ((out["color"] * _t(wc, False)).sum() + (out["normal_map"] * _t(wn, False)).sum() + (out["refl_strength_map"] * _t(wr, False)).sum() +
         (out["invdepth"] * _t(wi, False)).sum()).backward()
        res[option] = {k_: t[k_].grad.numpy() for k_ in ("means3D", "scales", "rotations")}
    vis = ref["radii"] > 0
    cx, cy = out["clamped_x"].numpy() & vis, out["clamped_y"].numpy() & vis
    gm = g["dL_dmeans3D"].reshape(P, 3)
    moved = np.abs(gm).max(axis=1) > 0
    assert (cx & ~cy & moved).sum() >= 5 and (cy & ~cx & moved).sum() >= 5 and (cx & cy & moved).sum() >= 5, (cx.sum(), cy.sum(), moved.sum())
    for k_, gk in dict(means3D="dL_dmeans3D", scales="dL_dscales", rotations="dL_drotations").items():
        _assert_close(g[gk].reshape(p[k_].shape), res[True][k_], 2e-6, gk + " (clamped coordinate held constant)")
    for k_, gk in dict(scales="dL_dscales", rotations="dL_drotations").items():
        _assert_close(g[gk].reshape(p[k_].shape), res[False][k_], 2e-6, gk + " (does not pass through dJ)")
    clamped = cx | cy
    scale = np.abs(res[False]["means3D"]).max()
    diff = np.abs(gm - res[False]["means3D"]).max(axis=1)
    assert diff[~clamped].max() <= 2e-6 * scale
    assert (diff[clamped & moved] > 1e-4 * scale).sum() >= 5, diff[clamped] / scale


def _truncating_camera(kind, seed):
    """The camera of _general_camera(kind) at the first (size, focal length) pairs near 48 x 32 for which int(focal * tan * 2) comes out
    one short IN DOUBLE, so that the float64 oracle takes the branch: (view, full, campos, tanx, tany, W, H), (Wb, Hb)."""
    t = trunc_search(40, 28, ratio=1.4, dtype=np.float64)
    w, h = t["W"], t["H"]
    cx, cy = (w / 2 + 0.15 * w, h / 2 - 0.12 * h) if kind == "all" else (w / 2, h / 2)
    R, T = rolled_pose(seed) if kind == "all" else (None, None)
    cam = hwk_camera(w, h, t["fx"], t["fy"], cx, cy, R, T)
    size = backward_size(w, cam["tanfovx"], np.float64), backward_size(h, cam["tanfovy"], np.float64)
    return (cam["viewmatrix"].astype(np.float64), cam["projmatrix"].astype(np.float64), cam["campos"].astype(np.float64), cam["tanfovx"],
            cam["tanfovy"], w, h), size


@pytest.mark.parametrize("kind", ["centred", "all"])
def test_surfel_backward_rebuilds_the_homography_for_a_truncated_image_size(kind):
    """DSR backward.cu:637-638: the per-surfel backward forms W' = int(focal_x * tan_fovx * 2), H' = int(focal_y * tan_fovy * 2) and
    rebuilds T from the inputs with ndc2pix(W', H').  At this camera both come out one short.  Known answer (dense_torch.render_surfel,
    backward_size): G = dL/dT of the TRUE forward, plus the bounding-box-centre term evaluated at T', pulled back to mean, scales and
    rotation through T' = [L0|0; L1|0; p|1] . PV . ndc2pix(W', H'); colour, normal and opacity paths as they are.  The oracle agrees with
    that at the tolerance of test_oracle_dense.py and differs from plain autograd by about 1 / W."""
    P = 48
    cam, (wb, hb) = _truncating_camera(kind, 4)
    view, full, campos, tanx, tany, w, h = cam
    assert (wb, hb) == (w - 1, h - 1)
    p = _in_view(_scene("S", P, 14), cam)
    bg = np.array([0.2, 0.5, 0.3])
    o = orc.SurfelOracle(np.float64)
    ref = o.forward(bg=bg, means3D=p["means3D"], opacities=p["opacities"], viewmatrix=view, projmatrix=full, campos=campos, tanfovx=tanx,
                    tanfovy=tany, image_height=h, image_width=w, sh_degree=3, shs=p["shs"], refl_strengths=p["refl_strengths"],
                    scales=p["scales"], rotations=p["rotations"], env_scope_mask=p["mask"])
    rs = np.random.RandomState(74)
    wc, wr, wa = rs.normal(size=(3, h, w)), rs.normal(size=(1, h, w)), rs.normal(size=(8, h, w))
    wa[7] = 0.0
    wa[6] *= 1e3
    g = o.backward(dL_dcolor=wc, dL_dallmap=wa, dL_drefl_strength_map=wr)
    res = {}
    for size in ((wb, hb), None):
        t = {k: _t(p[k]) for k in ("means3D", "scales", "rotations", "opacities", "shs", "refl_strengths")}
        out = dn.render_surfel(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["refl_strengths"],
                               torch.from_numpy(p["mask"].astype(np.float64)), _t(view, False), _t(full, False), _t(campos, False), tanx, tany, w, h,
                               _t(bg, False), freeze_lowpass_depth=True, backward_size=size)
        np.testing.assert_array_equal(out["radii"].numpy(), ref["radii"])
        _assert_close(out["color"].detach().numpy(), ref["color"], 1e-10, "color")
        assert out["lowpass_pairs"] > 50            # the bounding-box-centre term is live
        ((out["color"] * _t(wc, False)).sum() + (out["allmap"] * _t(wa, False)).sum() + (out["refl_strength_map"] * _t(wr, False)).sum()).backward()
        res[size is None] = {k: t[k].grad.numpy() for k in t}
    known, plain = res[False], res[True]
    q, ga = p["rotations"], g["dL_drotations"]
    tangential = ga - q * (q * ga).sum(axis=1, keepdims=True)
    for k, gk in dict(means3D="dL_dmeans3D", scales="dL_dscales", opacities="dL_dopacity", refl_strengths="dL_drefl_strengths", shs="dL_dsh").items():
        _assert_close(g[gk].reshape(p[k].shape), known[k], 1e-7, gk)
    _assert_close(tangential, known["rotations"], 1e-7, "dL_drotations (tangential)")
    for k, got in dict(means3D=g["dL_dmeans3D"].reshape(P, 3), scales=g["dL_dscales"], rotations=tangential).items():
        rel = np.abs(got - plain[k]).max() / np.abs(plain[k]).max()
        assert 0.1 / w < rel < 10.0 / w, (k, rel)
    for k, gk in dict(opacities="dL_dopacity", refl_strengths="dL_drefl_strengths", shs="dL_dsh").items():
        _assert_close(g[gk].reshape(p[k].shape), plain[k], 1e-7, gk + " (does not pass through T)")


def _surfel_pair(seed, log_scale):
    P = 24
    p = _scene("S", P, seed, log_scale=log_scale)
    view, full, campos = _camera(seed)
    bg = np.array([0.2, 0.5, 0.3])
    o = orc.SurfelOracle(np.float64)
    o.forward(bg=bg, means3D=p["means3D"], opacities=p["opacities"], viewmatrix=view, projmatrix=full, campos=campos, tanfovx=TAN, tanfovy=TAN,
              image_height=H, image_width=W, sh_degree=3, shs=p["shs"], refl_strengths=p["refl_strengths"], scales=p["scales"],
              rotations=p["rotations"], env_scope_mask=p["mask"])
    return p, view, full, campos, bg, o


def test_surfel_mean2d_is_overwritten_with_the_densification_signal():
    """DSR backward.cu:656-659: whatever the tile pass accumulated in dL_dmean2D is replaced by
        dL_dmean2D.x = dL_dtransMat[2] * transMat[8] * 0.5 * W,   .y = dL_dtransMat[5] * transMat[8] * 0.5 * H
    where dL_dtransMat is the gradient the TILE PASS accumulated (the per-pair use of T; the bounding-box-centre term is
    folded in later) and transMat[2], [5], [8] are the constant-term coefficients of x w, y w and w.  In the dense model
    T[:, i, j] is the coefficient of local coordinate i in output j, so these are T[:, 2, 0], T[:, 2, 1], T[:, 2, 2] and the
    pair-path gradient is d loss / d T with the centre detached."""
    p, view, full, campos, bg, o = _surfel_pair(11, -1.7)
    rs = np.random.RandomState(71)
    wc, wr, wa = rs.normal(size=(3, H, W)), rs.normal(size=(1, H, W)), rs.normal(size=(8, H, W))
    wa[7] = 0.0
    g = o.backward(dL_dcolor=wc, dL_dallmap=wa, dL_drefl_strength_map=wr)
    t = {k: _t(p[k]) for k in ("means3D", "scales", "rotations", "opacities", "shs", "refl_strengths")}
    out = dn.render_surfel(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["refl_strengths"],
                           torch.from_numpy(p["mask"].astype(np.float64)), _t(view, False), _t(full, False), _t(campos, False), TAN, TAN, W, H,
                           _t(bg, False), freeze_lowpass_depth=True, pair_path_only_T=True)
    ((out["color"] * _t(wc, False)).sum() + (out["allmap"] * _t(wa, False)).sum() + (out["refl_strength_map"] * _t(wr, False)).sum()).backward()
    Tm, dT = out["Tm"].detach().numpy(), out["Tm"].grad.numpy()
    visible = out["radii"].numpy() > 0
    expect = np.stack([dT[:, 2, 0] * Tm[:, 2, 2] * 0.5 * W, dT[:, 2, 1] * Tm[:, 2, 2] * 0.5 * H], axis=1) * visible[:, None]
    assert np.abs(expect).max() > 0
    _assert_close(g["dL_dmeans2D"][:, :2], expect, 1e-7, "dL_dmean2D (densification signal)")
    assert np.abs(g["dL_dmeans2D"][:, 2]).max() == 0


def test_surfel_lowpass_branch_freezes_the_intersection_point():
    """DSR backward.cu:454-464: where the low-pass falloff wins (rho2d < rho3d) the depth gradient is propagated with the
    ray-splat intersection point s held constant.  With small surfels (many such pairs) the oracle therefore agrees with the
    dense model that freezes s there (checked in test_oracle_dense.py) and DISAGREES with plain autograd."""
    p, view, full, campos, bg, o = _surfel_pair(12, -2.6)
    rs = np.random.RandomState(72)
    wa = np.zeros((8, H, W))
    wa[0] = rs.normal(size=(H, W))
    g = o.backward(dL_dcolor=np.zeros((3, H, W)), dL_dallmap=wa, dL_drefl_strength_map=np.zeros((1, H, W)))
    res = {}
    for freeze in (True, False):
        t = {k: _t(p[k]) for k in ("means3D", "scales", "rotations", "opacities", "shs", "refl_strengths")}
        out = dn.render_surfel(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["shs"], t["refl_strengths"],
                               torch.from_numpy(p["mask"].astype(np.float64)), _t(view, False), _t(full, False), _t(campos, False), TAN, TAN, W, H,
                               _t(bg, False), freeze_lowpass_depth=freeze)
        assert out["lowpass_pairs"] > 50
        (out["allmap"] * _t(wa, False)).sum().backward()
        res[freeze] = t["scales"].grad.numpy()
    _assert_close(g["dL_dscales"], res[True], 1e-7, "dL_dscales (frozen s)")
    assert np.abs(g["dL_dscales"] - res[False]).max() > 1e-3 * np.abs(res[False]).max()
