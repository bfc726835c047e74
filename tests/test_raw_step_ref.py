"""tests/raw_step_ref.py, the float64 restatement of the raw-parameter step (include/gsr_hip_train.h), pinned against torch's own chain in
float64: torch.sigmoid / exp / nn.functional.normalize, autograd, torch.optim.Adam(lr=0, eps=1e-15) with one lr per group, three steps.
No GPU and no library: this fixes the yardstick the GPU tests measure the kernel with.

Agreement is at float64 rounding, which is not one number for every element: the bound below is the first-order propagation of
K = 64 roundings (eps = 2^-52) through the chain, written out.
  * gradient: sigmoid's backward is g (1 - y) y with y rounded, so 1 - y carries an absolute error of eps and the gradient a relative one
    of eps / (1 - y) (5e8 eps at a logit of +20, where the restatement forms 1 / (1 + exp(r)) without that cancellation); normalize's
    g - q (q.g) cancels, so its error is absolute, eps |g_row| / |q|; exp and the plain groups round once.
  * moments: m and v are linear in the gradient and its square; the bounds follow the same recurrences.
  * parameter: u = m / (sqrt(v) / sqrt(bc2) + eps) takes dm / denom + |m| dv / (2 sqrt(v) sqrt(bc2) denom^2); the step adds lr / bc1 times that.
  * activated copy: its derivative (at most 1/4, the value itself, 1 / |q|) times the parameter's bound, plus one rounding."""
import numpy as np
import pytest
import torch

import raw_step_ref as R

EPS64 = 2.0 ** -52
K = 64.0
BETAS = (0.9, 0.999)


def _case(frozen):
    t, grads = R.make_case(7, scale_dims=2, L=2, M=4, seed=3, steps=3)
    t["opacities"][0], t["opacities"][1] = 20.0, -20.0          # saturated both ways
    t["refl_strengths"][2], t["refl_strengths"][3] = -20.0, 20.0
    for g in grads:                                              # (their gradients are not among the exact zeros)
        g["opacities"][:2] = [[1.5e-3], [-0.7e-3]]
        g["refl_strengths"][2:4] = [[-2e-3], [1e-3]]
    assert not t["rotations"][7 // 2].any()                      # the zero quaternion row of make_case
    lay = R.Layout(t)
    segs, n_act = R.segments_of(lay, R.default_groups(lay.names, 4), frozen=frozen)
    return t, grads, lay, segs, n_act


def _grad_bound(seg, r, g, rg):
    kind = seg.kind & 0xFF
    if kind == R.SIGMOID:
        return K * EPS64 * np.abs(rg) * (1.0 + (1.0 + np.exp(r)))          # 1 / (1 - a) = 1 + exp(r)
    if kind == R.NORMALIZE4:
        q, gg = r.reshape(-1, 4), g.reshape(-1, 4)
        row = np.sqrt((gg * gg).sum(axis=1)) / np.maximum(np.sqrt((q * q).sum(axis=1)), R.NORM_EPS)
        return np.repeat(K * EPS64 * row, 4)
    return K * EPS64 * np.abs(rg)


@pytest.mark.parametrize("frozen", [(), ("means3D", "rotations")], ids=["all-groups", "freeze_xyz"])
def test_restatement_matches_torch_float64_over_three_steps(frozen):
    t, grads, lay, segs, n_act = _case(frozen)
    raw0 = R.flat_from(lay, t, np.float64)
    gflat = [R.flat_from(lay, g, np.float64) for g in grads]
    chain = R.torch_chain((lay.names, lay.slices, lay.shapes, raw0), gflat, segs, 3, torch.float64, betas=BETAS)
    cur = dict(raw=raw0, m=np.zeros_like(raw0), v=np.zeros_like(raw0), act=R.activate(raw0, np.zeros(n_act), segs))
    dm, dv, dr = np.zeros_like(raw0), np.zeros_like(raw0), np.zeros_like(raw0)
    for step in range(1, 4):
        before = cur["raw"].copy()
        cur = R.step(cur["raw"], gflat[step - 1], cur["m"], cur["v"], cur["act"], segs, step, betas=BETAS)
        ref = chain[step - 1]
        acts = dict(ref["act"])
        bc1, sbc2 = 1.0 - BETAS[0] ** step, np.sqrt(1.0 - BETAS[1] ** step)
        for name, s in zip(lay.names, segs):
            a, b = lay.slices[name]
            if s.kind & R.FROZEN:
                for q in ("raw", "m", "v"):
                    assert np.array_equal(cur[q][a:b], ref[q][a:b]), (name, q)
                assert np.array_equal(cur["raw"][a:b], raw0[a:b]) and not cur["m"][a:b].any() and not cur["v"][a:b].any()
                continue
            rg = cur["raw_grad"][a:b]
            dg = _grad_bound(s, before[a:b], gflat[step - 1][a:b], rg)
            assert (np.abs(rg - ref["raw_grad"][a:b]) <= dg + 1e-300).all(), (name, step, "raw_grad")
            dm[a:b] = BETAS[0] * dm[a:b] + (1 - BETAS[0]) * dg + K * EPS64 * np.abs(cur["m"][a:b])
            dv[a:b] = BETAS[1] * dv[a:b] + (1 - BETAS[1]) * 2 * np.abs(rg) * dg + K * EPS64 * cur["v"][a:b]
            assert (np.abs(cur["m"][a:b] - ref["m"][a:b]) <= dm[a:b] + 1e-300).all(), (name, step, "m")
            assert (np.abs(cur["v"][a:b] - ref["v"][a:b]) <= dv[a:b] + 1e-300).all(), (name, step, "v")
            sv = np.sqrt(cur["v"][a:b])
            denom = sv / sbc2 + 1e-15
            du = dm[a:b] / denom + np.abs(cur["m"][a:b]) * np.where(sv > 0, dv[a:b] / np.maximum(2 * sv * sbc2, 1e-300), 0.0) / denom ** 2
            lr = R.element_lr(s)[:b - a]
            dr[a:b] = dr[a:b] + lr / bc1 * du + K * EPS64 * (np.abs(cur["raw"][a:b]) + lr)
            assert (np.abs(cur["raw"][a:b] - ref["raw"][a:b]) <= dr[a:b]).all(), (name, step, "raw")
            kind = s.kind & 0xFF
            if kind:
                mine = cur["act"][s.act_begin:s.act_begin + (b - a)]
                if kind == R.NORMALIZE4:
                    q = cur["raw"][a:b].reshape(-1, 4)
                    slope = np.repeat(4 * dr[a:b].reshape(-1, 4).max(axis=1) / np.maximum(np.sqrt((q * q).sum(axis=1)), R.NORM_EPS), 4)
                else:
                    slope = dr[a:b] * (0.25 if kind == R.SIGMOID else np.abs(mine))
                assert (np.abs(mine - acts[name]) <= slope + K * EPS64 * np.abs(mine)).all(), (name, step, "act")


def test_pinned_inputs_reach_the_edges():
    """What the pin must cover is in it: a zero quaternion row (gradient g / 1e-12), logits of +-20, the two learning rates inside every shs
    row, and a frozen group that nothing moves."""
    t, grads, lay, segs, n_act = _case(("means3D", "rotations"))
    raw0 = R.flat_from(lay, t, np.float64)
    g0 = R.flat_from(lay, grads[0], np.float64)
    seg = dict(zip(lay.names, segs))
    assert seg["shs"].period == 12 and seg["shs"].split == 3 and seg["shs"].lr2 == R.f32(0.0025 / 20.0)
    lr = R.element_lr(seg["shs"])
    assert (lr[:3] == seg["shs"].lr).all() and (lr[3:12] == seg["shs"].lr2).all() and lr[12] == seg["shs"].lr
    t2, _, lay2, segs2, _ = _case(())
    out = R.step(raw0, g0, np.zeros_like(raw0), np.zeros_like(raw0), np.zeros(n_act), segs2, 1)
    a, b = lay.slices["rotations"]
    z = a + 4 * (7 // 2)
    assert np.allclose(out["raw_grad"][z:z + 4], g0[z:z + 4] / 1e-12, rtol=1e-15)
    a, b = lay.slices["opacities"]
    assert 0 < out["raw_grad"][a] < 1e-11 and -1e-11 < out["raw_grad"][a + 1] < 0      # g a (1 - a) at +-20, not flushed to 0
    # step 1 moves every element with a non-zero gradient by its learning rate, sign(g): torch.optim.Adam's first step
    for name, s in zip(lay2.names, segs2):
        a, b = lay2.slices[name]
        nz = np.abs(out["raw_grad"][a:b]) > 1e-5            # (eps = 1e-15 in the denominator is then below 1e-10 of it)
        want = raw0[a:b] - R.element_lr(s)[:b - a] * np.sign(out["raw_grad"][a:b])
        assert np.allclose(out["raw"][a:b][nz], want[nz], rtol=0, atol=1e-9 * R.element_lr(s).max() + 1e-12), name
    # the activated copy of a sigmoid group stays inside (0, 1), of the scales positive, of the quaternions of unit length
    act = out["act"]
    for name, s in zip(lay2.names, segs2):
        n = lay2.slices[name][1] - lay2.slices[name][0]
        x = act[s.act_begin:s.act_begin + n]
        if (s.kind & 0xFF) == R.SIGMOID:
            assert ((x > 0) & (x < 1)).all()
        elif (s.kind & 0xFF) == R.EXP:
            assert (x > 0).all()
        elif (s.kind & 0xFF) == R.NORMALIZE4:
            assert np.allclose((x.reshape(-1, 4) ** 2).sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("P", [1, 3, 257, 1031])
@pytest.mark.parametrize("scale_dims", [2, 3])
def test_seeds_of_the_gpu_cases_keep_the_rotation_exemption_within_its_cap(P, scale_dims):
    """tests/test_gpu_raw_step.py may leave out at most 2 rotation elements per step: those whose float64 raw gradient is below 1e-5 of their
    row's incoming gradient norm (there the projection cancels and the sign Adam's first step takes is decided by rounding).  The seeds it
    uses keep the restatement itself within that cap; checked here, without a GPU."""
    t, grads = R.make_case(P, scale_dims=scale_dims, L=2, M=4, seed=R.seed_of(P, scale_dims), steps=3)
    lay = R.Layout(t)
    segs, n_act = R.segments_of(lay, R.default_groups(lay.names, 4))
    cur = dict(raw=R.flat_from(lay, t, np.float64), m=np.zeros(lay.total), v=np.zeros(lay.total), act=np.zeros(n_act))
    for step in range(1, 4):
        g = R.flat_from(lay, grads[step - 1], np.float64)
        cur = R.step(cur["raw"], g, cur["m"], cur["v"], cur["act"], segs, step)
        assert R.rotation_exempt(lay, cur["raw_grad"], g).sum() <= 2, (P, scale_dims, step)
