"""The flat layout's own answers on the host (gsr_train.FlatParams.segment, FlatAdam._segments / zero_moments, RawAdam's table,
GaussianTrainState.successor): everything here runs on device="cpu" and launches nothing.

Layouts: P in {1, 3, 257} (slices with and without padding), 1 to 3 shards (the last group carries the shard padding), with and without the
`cubemap` / `fail` groups behind the per-Gaussian ones."""
import types

import pytest
import torch

P_VALUES, SHARDS = (1, 3, 257), (1, 2, 3)
CASES = [(P, shards, env) for P in P_VALUES for shards in SHARDS for env in (False, True)]


def _tensors(P, env, M=4, S=2, L=2):
    g = torch.Generator().manual_seed(P)
    t = dict(means3D=torch.randn(P, 3, generator=g), shs=torch.randn(P, M, 3, generator=g), opacities=torch.randn(P, 1, generator=g),
             scales=torch.randn(P, S, generator=g), rotations=torch.randn(P, 4, generator=g), refl_strengths=torch.randn(P, 1, generator=g))
    if env:
        t.update(cubemap=torch.randn(6, 3, L, L, generator=g), fail=torch.randn(3, generator=g))
    return t


def _state(P, shards, env, rank=0):
    from gsr_train import GaussianTrainState
    return GaussianTrainState(_tensors(P, env), "cpu", shard=None if shards == 1 else (rank, shards))


@pytest.mark.parametrize("P,shards,env", CASES)
def test_segments_tile_the_buffer_in_group_order(hip_lib_built, P, shards, env):
    params = _state(P, shards, env).params
    assert params.total % (4 * shards) == 0
    at = 0
    for k in params.names:
        a, b = params.segment(k)
        assert a == at and a % 4 == 0, (k, a, at)
        assert a == params.slices[k][0] and params.slices[k][1] <= b < params.slices[k][1] + 4 * shards, (k, a, b)
        at = b
    assert at == params.total


@pytest.mark.parametrize("P,shards,env", CASES)
def test_both_optimizer_tables_agree_with_segment(hip_lib_built, P, shards, env):
    import _gsr
    from gsr_train import ACTIVATIONS, RawTrainState
    st = _state(P, shards, env)
    params, opt = st.params, st.optimizer
    opt.set_lr("means3D", 3e-5)
    plain = opt._segments()
    assert isinstance(plain, _gsr.AdamSegment * len(params.names))
    for k, s in zip(params.names, plain):
        assert (s.begin, s.end) == params.segment(k), k
        want = _gsr.AdamSegment(*params.segment(k), *opt.groups[k])
        assert all(getattr(s, f) == getattr(want, f) for f, _ in _gsr.AdamSegment._fields_), k
    # the table RawAdam builds (constructed as RawTrainState constructs it, never stepped)
    raw = RawTrainState._make_optimizer(types.SimpleNamespace(params=params, grads=st.grads, ACTIVATED=RawTrainState.ACTIVATED), dict(opt.groups), None)
    raw.frozen = {"means3D", "rotations"}
    table, at = raw._act_segments(), 0
    assert isinstance(table, _gsr.ActSegment * len(params.names))
    for k, s, p in zip(params.names, table, plain):
        assert all(getattr(s, f) == getattr(p, f) for f, _ in _gsr.AdamSegment._fields_), k
        kind = ACTIVATIONS[k] if k in RawTrainState.ACTIVATED else _gsr.GSR_ACT_NONE
        assert s.kind == kind | (_gsr.GSR_ACT_FROZEN if k in raw.frozen else 0), k
        if kind:
            assert s.act_begin == at and at % 4 == 0 and raw.act_slices[k] == (at, at + s.end - s.begin), k
            at += s.end - s.begin
        else:
            assert s.act_begin == 0, k
    assert raw.act.numel() == max(at, 4)


@pytest.mark.parametrize("P,shards,env", CASES)
def test_zero_moments_touches_the_owned_part_of_the_segment_alone(hip_lib_built, P, shards, env):
    for rank in range(shards):
        st = _state(P, shards, env, rank)
        params, opt = st.params, st.optimizer
        lo, hi = opt.owned
        assert (lo, hi) == (rank * params.total // shards, (rank + 1) * params.total // shards) and opt.exp_avg.numel() == hi - lo
        for k in params.names:
            opt.exp_avg.fill_(1.0)
            opt.exp_avg_sq.fill_(2.0)
            opt.zero_moments(k)
            a, b = params.segment(k)
            inside = torch.zeros(params.total, dtype=torch.bool)
            inside[a:b] = True
            inside = inside[lo:hi]
            assert torch.equal(opt.exp_avg == 0, inside) and torch.equal(opt.exp_avg[~inside], torch.ones(int((~inside).sum()))), (k, rank)
            assert torch.equal(opt.exp_avg_sq == 0, inside) and torch.equal(opt.exp_avg_sq[~inside], torch.full((int((~inside).sum()),), 2.0)), (k, rank)


@pytest.mark.parametrize("shards", SHARDS)
def test_successor_carries_the_optimizer_settings_and_the_shard(hip_lib_built, shards):
    from gsr_train import GaussianTrainState
    st = GaussianTrainState(_tensors(257, True), "cpu", spatial_lr_scale=2.5, lrs=dict(opacity_lr=0.03), shard=None if shards == 1 else (shards - 1, shards))
    opt = st.optimizer
    opt.betas, opt.eps, opt.step_count = (0.8, 0.99), 1e-8, 7
    st.update_learning_rate(1234)
    shapes = {k: ((300,) + v[1:] if k not in ("cubemap", "fail") else v) for k, v in st.params.shapes.items()}
    shapes["cubemap"] = (6, 3, 4, 4)
    new = st.successor(shapes)
    assert type(new) is type(st) and new is not st and new.params.shapes == shapes and new.params.names == st.params.names
    assert new.shard == st.shard and new.spatial_lr_scale == 2.5 and new.lrs == st.lrs
    assert new.params.total % (4 * shards) == 0
    n = new.params.total // shards
    assert new.optimizer.owned == ((shards - 1) * n, shards * n)
    assert (new.optimizer.betas, new.optimizer.eps, new.optimizer.step_count) == ((0.8, 0.99), 1e-8, 7)
    assert new.optimizer.groups == opt.groups and new.optimizer.groups is not opt.groups
    assert new.optimizer.groups["means3D"][0] == st.xyz_scheduler_args(1234) != st.lrs["position_lr_init"] * 2.5
    assert new.optimizer.groups["opacities"][0] == 0.03
    assert not new.params.flat.any() and not new.optimizer.exp_avg.any() and not new.grads.flat.any()
