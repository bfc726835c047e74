"""tests/env_scope_ref.py, the float64 restatement of the env-scope pass and of dist_color, pinned against the torch expressions it
restates (evaluated with float32 torch on the CPU), and its point generators held to what they promise.  No GPU."""
import numpy as np
import pytest
import torch

import env_scope_ref as E

ULP = 2.0 ** -23


def _torch_masks(xyz, centre, radius):
    """The two torch expressions as the reference and render() write them (float32)."""
    x = torch.from_numpy(xyz)
    c = torch.tensor([float(v) for v in centre])
    outside = torch.sum((x - c[None]) ** 2, dim=-1) > radius ** 2
    inside = ((x - c[None]) ** 2).sum(dim=-1) < radius ** 2
    return inside.numpy(), outside.numpy()


@pytest.mark.parametrize("P", [1, 2, 65, 1000, 4097])
def test_clear_points_have_an_empty_band_and_populate_both_masks(P):
    xyz, refl, c, r = E.clear_points(P, seed=P)
    assert xyz.dtype == np.float32 and xyz.shape == (P, 3) and refl.shape == (P,)
    assert not E.band(xyz, c, r).any()
    inside, outside = E.masks(xyz, c, r)
    assert not (inside & outside).any() and (inside | outside).all()
    even = np.arange(P) % 2 == 0
    assert (inside == even).all() and (outside == ~even).all()
    d = np.sqrt(E.d2(xyz, c))
    assert (d[even] <= 0.98 * r * (1 + 1e-6)).all() and (d[~even] >= 1.02 * r * (1 - 1e-6)).all() and (d <= 3 * r * (1 + 1e-6)).all()
    if P >= 65:
        assert inside.sum() >= 0.3 * P and outside.sum() >= 0.3 * P
    ti, to = _torch_masks(xyz, c, r)
    assert (ti == inside).all() and (to == outside).all()


def test_shell_points_lie_outside_the_band_on_the_intended_side():
    xyz, refl, c, r, side = E.shell_points(4097)
    assert not E.band(xyz, c, r).any()
    inside, outside = E.masks(xyz, c, r)
    assert (inside == (side < 0)).all() and (outside == (side > 0)).all()
    q, r2 = E.d2(xyz, c), E.radius2(r)
    rel = np.abs(q - r2) / r2
    assert rel.max() < 2.0 ** -16 and rel.min() > 2 * E.BAND       # on the shell, and at least two band widths off the sphere
    ti, to = _torch_masks(xyz, c, r)
    assert (ti == inside).all() and (to == outside).all()


def test_lattice_points_sit_exactly_on_the_sphere_or_clearly_off_it():
    xyz, refl, c, r, want_in, want_out = E.lattice_points()
    q = E.d2(xyz, c)
    assert (q[:4] == 9.0).all() and q[4] == 8.0 and q[5] == 12.0 and np.isnan(q[6]) and np.isposinf(q[7])
    assert E.radius2(r) == 9.0
    inside, outside = E.masks(xyz, c, r)
    assert (inside == want_in).all() and (outside == want_out).all()
    assert not inside[:4].any() and not outside[:4].any() and not inside[6] and not outside[6] and outside[7] and not inside[7]
    ti, to = _torch_masks(xyz, c, r)
    assert (ti == want_in).all() and (to == want_out).all()
    # exact in float32 in any order of evaluation: every partial result is a small integer
    x32 = xyz[:6] - np.asarray(c, dtype=np.float32)[None]
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        s = np.float32(0)
        for k in order:
            s = np.float32(s + x32[:, k] * x32[:, k])
        assert (s.astype(np.float64) == q[:6]).all()


def test_band_brackets_the_float32_evaluation():
    """Where float32 torch and the float64 restatement disagree about a mask, the point is in the band (points drawn ON the sphere up to
    float32 rounding, where they do disagree), and the band is narrow: it holds no point of relative distance 1e-6 from the sphere."""
    rs = np.random.RandomState(3)
    c, r = E.CLEAR_CENTRE, E.CLEAR_RADIUS
    v = rs.standard_normal((20000, 3))
    xyz = (np.asarray(c)[None] + r * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    inside, outside = E.masks(xyz, c, r)
    ti, to = _torch_masks(xyz, c, r)
    differ = (ti != inside) | (to != outside)
    assert differ.any()
    assert E.band(xyz, c, r)[differ].all()
    off = (np.asarray(c)[None] + r * (1 + 1e-6) * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    assert not E.band(off, c, r).any()
    assert E.radius2(r) == float(torch.tensor(r ** 2, dtype=torch.float32)) and E.radius2(r) != r ** 2
    assert (E.centre32(c) == torch.tensor(list(c)).double().numpy()).all()


def test_loss_and_gradient_against_torch():
    xyz, refl, c, r = E.clear_points(1000, seed=5)
    inside, outside = E.masks(xyz, c, r)
    s, n, mean = E.loss(refl, outside)
    assert n == int(outside.sum()) and n > 0
    t = torch.from_numpy(refl)[:, None].clone().requires_grad_(True)         # [P,1], as get_refl
    x = torch.from_numpy(xyz)
    cen = torch.tensor([float(v) for v in c])
    msk = torch.sum((x - cen[None]) ** 2, dim=-1) > r ** 2
    val = t[msk].mean()
    (0.4 * val).backward()
    assert abs(float(val.detach()) - mean) <= n * E.U * s / n + ULP * mean          # any float32 summation order of n terms, and the division
    g = E.gradient(outside, 0.4)
    got = t.grad.numpy().reshape(-1).astype(np.float64)
    assert (got[~outside] == 0).all() and (g[~outside] == 0).all()
    assert np.abs(got[outside] - g[outside]).max() <= 2 * ULP * 0.4 / n
    # an empty selection: NaN value, no gradient to any row
    none = np.zeros(1000, dtype=bool)
    assert np.isnan(E.loss(refl, none)[2]) and not E.gradient(none).any()
    t2 = torch.from_numpy(refl).clone().requires_grad_(True)
    v2 = t2[torch.from_numpy(none)].mean()
    v2.backward()
    assert torch.isnan(v2) and not t2.grad.any()


def test_dist_color_against_torch():
    rs = np.random.RandomState(7)
    P = 501
    dc = rs.standard_normal((P, 1, 3)).astype(np.float32)
    noise = rs.rand(P, 1, 3).astype(np.float32)
    msk = rs.rand(P) < 0.4
    want = E.dist_color(dc, noise, 0.4, msk)
    dcc = torch.from_numpy(dc).clone()                                       # gaussian_model.py:279-282 with the noise given
    dist_dcc = dcc + (torch.from_numpy(noise) * 0.4 * 2 - 0.4)
    dist_dcc[torch.from_numpy(msk)] = dcc[torch.from_numpy(msk)]
    got = dist_dcc.numpy().reshape(P, 3).astype(np.float64)
    assert (got[msk] == dc.reshape(P, 3)[msk]).all() and (want[msk] == dc.reshape(P, 3)[msk]).all()
    assert np.abs(got - want).max() <= 4 * ULP * max(1.0, np.abs(want).max())
    assert (np.abs(want[~msk] - dc.reshape(P, 3)[~msk]) <= 0.4 + 1e-12).all() and (want[~msk] != dc.reshape(P, 3)[~msk]).any()
