"""Flat Adam step through the C ABI (gsr_adam_step_range, csrc/gsr_train.hip) at the edges its callers in this package never
reach: segment boundaries at every residue mod 4 (the per-element learning rate inside one float4), exactly 16 segments and
empty ones, interleaved rates with split 0 / period and a period that is not a multiple of 4, sizes 1, 3, 5 and 1e6 + 3, a
range starting past 0 with a ragged end, zero gradients (denominator = eps), and the step counters 1, 2 and 30 000.
Against the float64 oracle within the bounds of tests/loss_bounds.py, and against torch.optim.Adam on the device within a
few ulp."""
import numpy as np
import pytest
import torch

import loss_bounds as LB

pytestmark = pytest.mark.gpu
B1, B2, EPS = 0.9, 0.999, 1e-15


def lr_per_element(segs, n):
    """The learning rate each element gets, from the segment list as include/gsr_hip.h documents it."""
    lr = np.zeros(n, np.float32)
    for (b, e, r1, r2, period, split) in segs:
        i = np.arange(b, e)
        lr[b:e] = r1 if period == 0 else np.where((i - b) % period < split, r1, r2)
    return lr


def run_adam(state, segs, step, rb=0, re=None):
    from _gsr import AdamSegment, check, lib
    p, g, m, v = (torch.from_numpy(np.ascontiguousarray(t, np.float32)).cuda() for t in state)
    n = p.numel()
    re = n if re is None else re
    arr = (AdamSegment * len(segs))(*[AdamSegment(b, e, r1, r2, period, split) for (b, e, r1, r2, period, split) in segs])
    check(lib.gsr_adam_step_range(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, arr, len(segs), B1, B2, EPS, step, rb, re, None),
          "gsr_adam_step_range")
    torch.cuda.synchronize()
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def make_state(n, seed, zero_grad=False, fresh=False):
    rs = np.random.RandomState(seed)
    p = rs.randn(n).astype(np.float32)
    g = np.zeros(n, np.float32) if zero_grad else (rs.randn(n) * 10.0 ** rs.uniform(-6, 1, n)).astype(np.float32)
    m = np.zeros(n, np.float32) if fresh else (rs.randn(n) * 0.1).astype(np.float32)
    v = np.zeros(n, np.float32) if fresh or zero_grad else (rs.rand(n) * 0.01).astype(np.float32)
    return p, g, m, v


def check_adam(state, segs, step, rb=0, re=None, what=""):
    n = state[0].size
    re = n if re is None else re
    got = run_adam(state, segs, step, rb, re)
    ref, bnd = LB.adam_reference(*state, lr_per_element(segs, n), B1, B2, EPS, step)
    for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        LB.check(got[k][rb:re], ref[k][rb:re], bnd[k][rb:re], what=f"{what} {name}")
        assert np.array_equal(got[k][:rb], state[(0, 2, 3)[k]][:rb]) and np.array_equal(got[k][re:], state[(0, 2, 3)[k]][re:]), what
    return got


def torch_adam(state, lr, step):
    """torch.optim.Adam on the device, one call at `step` from the given moments."""
    p, g, m, v = (torch.from_numpy(np.ascontiguousarray(t, np.float32)).cuda() for t in state)
    w = p.clone().requires_grad_(True)
    f32 = lambda t: float(np.float32(t))          # the values the C ABI receives: the same operation, not Python-double betas
    opt = torch.optim.Adam([w], lr=f32(lr), betas=(f32(B1), f32(B2)), eps=f32(EPS))
    opt.state[w] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    w.grad = g
    opt.step()
    st = opt.state[w]
    return w.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()


@pytest.mark.parametrize("step", [1, 2, 30_000])
def test_sixteen_segments_at_every_residue(step):
    """16 segments whose boundaries fall on every residue mod 4, three of them empty, each with its own learning rate."""
    ends = [1, 2, 3, 4, 4, 9, 14, 19, 24, 24, 31, 37, 38, 38, 43, 50]
    segs, b = [], 0
    for k, e in enumerate(ends):
        segs.append((b, e, 1e-3 * (k + 1), 0.0, 0, 0))
        b = e
    assert len(segs) == 16 and {e % 4 for e in ends} == {0, 1, 2, 3}
    check_adam(make_state(ends[-1], step), segs, step, what=f"step {step}")


@pytest.mark.parametrize("split", ["zero", "period", "inner"])
def test_interleaved_rates(split):
    period = 7
    sp = {"zero": 0, "period": period, "inner": 3}[split]
    n = 7 * 13 + 5
    segs = [(0, 6, 0.01, 0.0, 0, 0), (6, 6 + 7 * 12, 0.0025, 0.0025 / 20, period, sp), (6 + 7 * 12, n, 0.05, 0.0, 0, 0)]
    check_adam(make_state(n, 3), segs, 2, what=split)


@pytest.mark.parametrize("n", [1, 3, 5, 1_000_003])
def test_sizes(n):
    segs = [(0, n // 2, 0.01, 0.0, 0, 0), (n // 2, n, 0.002, 0.0, 0, 0)] if n > 1 else [(0, 1, 0.01, 0.0, 0, 0)]
    state = make_state(n, n)
    got = check_adam(state, segs, 3, what=f"n={n}")
    # torch.optim.Adam on the device, one parameter group per segment: both are float32 evaluations of the same step (torch
    # arranges it as lerp / addcmul / addcdiv), so each lies within the bound of the float64 step and they differ by at most
    # twice it, a few ulp of the terms involved
    _, bnd = LB.adam_reference(*state, lr_per_element(segs, n), B1, B2, EPS, 3)
    for (b, e, lr, _, _, _) in segs:
        if e == b:
            continue
        for k, t in enumerate(torch_adam([t[b:e] for t in state], lr, 3)):
            assert (np.abs(got[k][b:e].astype(np.float64) - t) <= 2 * bnd[k][b:e]).all(), (n, k)


def test_range_past_zero_with_ragged_end():
    """One rank's shard [range_begin, n) of the flat buffer: elements before it are left untouched bit for bit."""
    n = 1_000_003
    segs = [(0, 300_001, 0.01, 0.0, 0, 0), (300_001, 700_002, 0.002, 0.0003, 48, 3), (700_002, n, 0.05, 0.0, 0, 0)]
    state = make_state(n, 5)
    check_adam(state, segs, 2, rb=400_000, re=n, what="shard")
    check_adam(state, segs, 2, rb=700_000, re=700_008, what="inner shard")


@pytest.mark.parametrize("step", [1, 30_000])
def test_zero_gradients(step):
    """g = 0: with fresh moments nothing moves; with m != 0 and v = 0 the denominator is eps and the step is m / eps."""
    n = 37
    segs = [(0, 17, 0.01, 0.0, 0, 0), (17, n, 1e-20, 0.0, 0, 0)]
    p, g, m, v = make_state(n, 9, zero_grad=True, fresh=True)
    got = check_adam((p, g, m, v), segs, step, what="fresh")
    assert np.array_equal(got[0], p)
    p, g, m, v = make_state(n, 9, zero_grad=True)
    assert (v == 0).all() and (m != 0).all()
    check_adam((p, g, m, v), segs, step, what="v = 0")
