"""The densification plan on the device (include/gsr_hip_densify.h; gsr_densify.densify_and_prune(plan="device"), gsr_densify.prune_points)
on the GPU.  The yardstick is plan="torch" — the host-composed plan, bit for bit: the fixtures (tests/densify_fixtures.py) keep every
largest scale and every squared distance 1e-5 relative away from its threshold, which is where the two plans' expf and three-term sums
could round to different sides; the weight and gradient tests are IEEE divisions of identical inputs — and, for the seeded fixture of
tests/test_gpu_densify.py, the numpy restatement of the reference (oracle/oracle_densify.py) under that file's comparisons.

The classify kernels rank B = 256 rows per workgroup (PLAN_B of csrc/gsr_densify.hip) and the count scan takes 256 workgroups per turn,
C = 65536 rows: the shapes below run through 1, 2, one wave +- 1, B - 1, B, B + 1, 2 B + 1 and C + 1."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import densify_fixtures as F

pytestmark = pytest.mark.gpu

STATE_SEED = 17


def _state(fx, raw=False, shard=None):
    import gsr_synth as S
    from gsr_train import GaussianTrainState, RawTrainState
    tex, fail = S.make_cubemap(8, 3, STATE_SEED)
    tensors = {k: torch.from_numpy(fx["scene"][k]) for k in F.GROUPS}
    tensors["cubemap"], tensors["fail"] = torch.from_numpy(tex), torch.from_numpy(fail)
    st = RawTrainState(tensors, "cuda") if raw else GaussianTrainState(tensors, "cuda", shard=shard)
    if shard is None:
        g = torch.Generator(device="cpu").manual_seed(STATE_SEED)
        st.optimizer.exp_avg.copy_(torch.randn(st.params.total, generator=g))
        st.optimizer.exp_avg_sq.copy_(torch.rand(st.params.total, generator=g))
    st.optimizer.step_count, st.optimizer.betas, st.optimizer.eps = 17, (0.8, 0.99), 1e-8
    return st


def _stats(fx):
    from gsr_densify import DensifyStats
    s = DensifyStats(fx["P"], "cuda")
    s.buf.copy_(torch.from_numpy(np.stack([fx["stats"][k] for k in F.STAT_NAMES])))
    return s


def _noise(fx):
    k = int(F.classes(fx)[2].sum())
    return fx["noise_pool"][:fx["N"] * k]


def _run(fx, st, plan, screen, stats=None):
    from gsr_densify import densify_and_prune
    return densify_and_prune(st, stats if stats is not None else _stats(fx), F.MAX_GRAD, F.MIN_OPACITY, torch.tensor(fx["mean"]), fx["extent"], screen,
                             noise=torch.from_numpy(_noise(fx)).cuda(), plan=plan)


def _assert_same(got, want):
    """Two (new_state, new_stats, info) results: every parameter group, the whole flat buffers, both moment buffers, the fresh statistics
    and info."""
    (a, sa, ia), (b, sb, ib) = got, want
    assert ia == ib, (ia, ib)
    assert type(a) is type(b) and a.params.names == b.params.names and a.params.shapes == b.params.shapes and a.shard == b.shard
    for k in a.params.names:
        assert torch.equal(a.p[k].detach(), b.p[k].detach()), k
    assert torch.equal(a.params.flat, b.params.flat)
    assert torch.equal(a.optimizer.exp_avg, b.optimizer.exp_avg) and torch.equal(a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq)
    assert torch.equal(sa.buf, sb.buf) and float(sa.buf.abs().max() if sa.buf.numel() else 0.0) == 0.0
    oa, ob = a.optimizer, b.optimizer
    assert (oa.step_count, oa.betas, oa.eps, oa.groups, oa.owned) == (ob.step_count, ob.betas, ob.eps, ob.groups, ob.owned)


_shared = {}


def _both(key, screen, raw=False):
    """(fixture, old state, result of plan="torch", result of plan="device"), computed once per (fixture, threshold, class) and left alone."""
    if (key, screen, raw) not in _shared:
        fx = F.get(key)
        st = _state(fx, raw=raw)
        _shared[(key, screen, raw)] = (fx, st, _run(fx, st, "torch", screen), _run(fx, st, "device", screen))
    return _shared[(key, screen, raw)]


def _views(st, flat):
    return {k: st.params.view_of(flat, k).detach().cpu().numpy().copy() for k in F.GROUPS}


# ------------------------------------------------------------------------------------------------- equality with the torch plan and the oracle
@pytest.mark.parametrize("screen", [None, 20])
def test_device_plan_equals_torch_plan_and_the_oracle(screen):
    from oracle import oracle_densify as od
    fx, st, want, got = _both(F.MAIN, screen)
    _assert_same(got, want)
    new_state, new_stats, info = got
    s = F.summary(fx)
    assert (info["pruned_by_weight"], info["cloned"], info["split"], info["before"]) == (s["pruned"], s["cloned"], s["split"], fx["P"])
    assert min(info["pruned_by_weight"], info["cloned"], info["split"]) > 100
    assert info["pruned_big"] == (s["big"] if screen else 0) and info["after"] == s["length"] - info["pruned_big"]
    if screen:
        assert info["pruned_big"] > 0
    # the reference's sequence, operation by operation (the comparisons of tests/test_gpu_densify.py)
    mdl = od.Model(_views(st, st.params.flat), _views(st, st.optimizer.exp_avg), _views(st, st.optimizer.exp_avg_sq), fx["stats"])
    nc, ns = mdl.densify_and_prune(F.MAX_GRAD, F.MIN_OPACITY, np.asarray(fx["mean"], np.float32), fx["extent"], screen, _noise(fx))
    assert (info["cloned"], info["split"]) == (nc, ns)
    P1 = mdl.p["means3D"].shape[0]
    assert info["after"] == P1 and new_state.p["means3D"].shape[0] == P1
    got_p, got_m, got_v = (_views(new_state, b) for b in (new_state.params.flat, new_state.optimizer.exp_avg, new_state.optimizer.exp_avg_sq))
    for kk in ("shs", "opacities", "rotations", "refl_strengths"):
        np.testing.assert_array_equal(got_p[kk], mdl.p[kk].reshape(got_p[kk].shape))
    np.testing.assert_allclose(got_p["means3D"], mdl.p["means3D"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got_p["scales"], mdl.p["scales"], rtol=1e-5, atol=1e-6)
    for kk in F.GROUPS:
        np.testing.assert_array_equal(got_m[kk], mdl.m[kk].reshape(got_m[kk].shape))
        np.testing.assert_array_equal(got_v[kk], mdl.v[kk].reshape(got_v[kk].shape))
    assert torch.equal(new_state.p["cubemap"].detach(), st.p["cubemap"].detach()) and new_state.optimizer.step_count == 17
    assert float(new_stats.buf.abs().max()) == 0 and new_stats.buf.shape == (5, P1)


def test_the_new_state_takes_an_adam_step():
    fx = F.get(F.MAIN)
    new_state = _run(fx, _state(fx), "device", 20)[0]
    new_state.grads.flat.normal_()
    before = new_state.params.flat.clone()
    new_state.optimizer.step()
    assert torch.isfinite(new_state.params.flat).all() and not torch.equal(before, new_state.params.flat)
    assert new_state.optimizer.step_count == 18


def test_raw_train_state_stays_one_with_its_activated_copy_refreshed():
    from gsr_train import RawTrainState
    from poison import u32
    fx, st, want, got = _both(F.MAIN, 20, raw=True)
    _assert_same(got, want)
    new = got[0]
    assert type(new) is RawTrainState
    assert torch.equal(new.optimizer.act, want[0].optimizer.act)
    have = new.optimizer.act.clone()
    new.optimizer.act.fill_(float("nan"))
    new.optimizer.activate()
    torch.cuda.synchronize()
    assert u32(have.cpu().numpy()).tobytes() == u32(new.optimizer.act.cpu().numpy()).tobytes()


# ------------------------------------------------------------------------------------------------- the smallest shapes that can go wrong
@pytest.mark.parametrize("key", F.SMALL, ids=lambda k: "P%d" % k[0])
def test_shapes_around_the_wave_the_workgroup_and_the_scan_chunk(key):
    fx, st, want, got = _both(key, 20)
    _assert_same(got, want)
    assert got[2]["after"] >= 1
    if fx["P"] > 2000:
        assert min(got[2]["cloned"], got[2]["split"], got[2]["pruned_by_weight"], got[2]["pruned_big"]) > 0


# ------------------------------------------------------------------------------------------------- class mixes
def test_mix_nothing_selected_nothing_pruned_is_the_identity():
    fx, st, want, got = _both(F.MIXES[0], None)
    _assert_same(got, want)
    new, _, info = got
    assert info == dict(pruned_by_weight=0, cloned=0, split=0, pruned_big=0, before=300, after=300)
    assert torch.equal(new.params.flat, st.params.flat)
    for k in st.params.names:          # (group by group: the padding between groups carries no moments)
        for a, b in ((new.optimizer.exp_avg, st.optimizer.exp_avg), (new.optimizer.exp_avg_sq, st.optimizer.exp_avg_sq)):
            assert torch.equal(new.params.view_of(a, k), st.params.view_of(b, k)), k


def test_mix_every_row_a_clone():
    fx, st, want, got = _both(F.MIXES[1], 20)
    _assert_same(got, want)
    new, _, info = got
    assert info == dict(pruned_by_weight=0, cloned=300, split=0, pruned_big=0, before=300, after=600)
    for k in F.GROUPS:
        assert torch.equal(new.p[k].detach()[:300], st.p[k].detach()) and torch.equal(new.p[k].detach()[300:], st.p[k].detach()), k
        m = new.params.view_of(new.optimizer.exp_avg, k)
        assert torch.equal(m[:300], st.params.view_of(st.optimizer.exp_avg, k)) and float(m[300:].abs().max()) == 0.0, k


def test_mix_every_child_dropped_as_big_a_few_unsplit_rows_remain():
    fx, st, want, got = _both(F.MIXES[2], 20)
    _assert_same(got, want)
    new, _, info = got
    assert info == dict(pruned_by_weight=0, cloned=0, split=295, pruned_big=590, before=300, after=5)
    few = torch.arange(5) * 60 + 3
    assert torch.equal(new.p["means3D"].detach().cpu(), st.p["means3D"].detach().cpu()[few])


def test_mix_all_but_one_row_pruned_by_weight():
    fx, st, want, got = _both(F.MIXES[3], 20)
    _assert_same(got, want)
    new, _, info = got
    assert info == dict(pruned_by_weight=299, cloned=0, split=0, pruned_big=0, before=300, after=1)
    assert torch.equal(new.p["shs"].detach(), st.p["shs"].detach()[151:152])


def test_zero_denominators_classify_as_in_torch():
    fx, st, want, got = _both(F.DENOMS, 20)
    _assert_same(got, want)
    info, s = got[2], F.summary(fx)
    assert (info["pruned_by_weight"], info["cloned"], info["split"], info["pruned_big"]) == (s["pruned"], s["cloned"], s["split"], s["big"])
    # the rows set by hand: 8..23 (0 / 0) stay once, 24..31 (x / 0 = inf, small) are cloned, 32..39 (inf, large) are split, 40..55 (denom_w == 0) go
    old_xyz, new_xyz = st.p["means3D"].detach().cpu(), got[0].p["means3D"].detach().cpu()
    times = lambda r: int((new_xyz == old_xyz[r]).all(dim=1).sum())
    assert [times(r) for r in (8, 23)] == [1, 1] and [times(r) for r in (24, 31)] == [2, 2]
    assert [times(r) for r in (32, 39, 40, 55)] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------- degenerate counts at the C ABI
FILL = -7


def _cabi_plan(fx, screen=True, spare=10):
    """select -> split children -> rows on raw buffers through ctypes.  Every output is filled with FILL first."""
    from _gsr import DensifyPlan, check, lib
    P, N, e = fx["P"], fx["N"], fx["extent"]
    dev = "cuda"
    stats = {k: torch.from_numpy(fx["stats"][k]).to(dev) for k in F.STAT_NAMES}
    xyz, scaling, rot = (torch.from_numpy(fx["scene"][k]).to(dev) for k in ("means3D", "scales", "rotations"))
    plan = DensifyPlan(F.MAX_GRAD, F.MIN_WEIGHT, F.PERCENT_DENSE * e, 0.1 * e, 1.5 * e, e ** 2, (ctypes.c_float * 3)(*fx["mean"]), int(screen), N, 2)
    nbytes = int(lib.gsr_densify_plan_scratch_bytes(P, N))
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    sel = torch.full((4,), FILL, dtype=torch.int32, device=dev)
    parents = torch.full((P,), FILL, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    check(lib.gsr_densify_plan_select(P, ctypes.byref(plan), stats["xyz_gradient_accum"].data_ptr(), stats["denom"].data_ptr(), stats["accum_w"].data_ptr(),
                                      stats["denom_w"].data_ptr(), scaling.data_ptr(), scratch.data_ptr(), nbytes, sel.data_ptr(), parents.data_ptr(), stream),
          "gsr_densify_plan_select")
    survivors, clones, k, zero = sel.tolist()
    assert zero == 0
    length = survivors - k + clones + N * k
    child_xyz, child_scaling = torch.zeros(max(N * k, 1), 3, device=dev), torch.zeros(max(N * k, 1), 2, device=dev)
    if k:
        noise = torch.from_numpy(fx["noise_pool"][:N * k]).to(dev)
        check(lib.gsr_split_children(N * k, 2, N, parents[:k].repeat(N).data_ptr(), xyz.data_ptr(), scaling.data_ptr(), rot.data_ptr(), noise.data_ptr(),
                                     child_xyz.data_ptr(), child_scaling.data_ptr(), stream), "gsr_split_children")
    maps = torch.full((3, length + spare), FILL, dtype=torch.int32, device=dev)
    rows = torch.full((4,), FILL, dtype=torch.int32, device=dev)
    when_k = lambda t: t.data_ptr() if k else None
    check(lib.gsr_densify_plan_rows(P, ctypes.byref(plan), scratch.data_ptr(), nbytes, xyz.data_ptr(), scaling.data_ptr(), when_k(parents),
                                    when_k(child_xyz), when_k(child_scaling), k, maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(),
                                    rows.data_ptr(), stream), "gsr_densify_plan_rows")
    return sel.tolist(), parents.cpu(), rows.tolist(), maps.cpu(), length


def test_cabi_no_survivor_no_clone_no_parent():
    P = 300
    # survivors = 0: every row pruned by weight
    fx = dict(F.get(F.MIXES[3]))
    fx["stats"] = dict(fx["stats"], accum_w=np.zeros(P, np.float32))
    sel, parents, rows, maps, length = _cabi_plan(fx)
    assert sel == [0, 0, 0, 0] and rows == [0, 0, 0, 0] and length == 0
    assert bool((parents == FILL).all()) and bool((maps == FILL).all())
    # clones = 0 and k = 0: the survivors in place, no entry of the clone or child segments
    sel, parents, rows, maps, length = _cabi_plan(F.get(F.MIXES[0]), screen=False)
    assert sel == [P, 0, 0, 0] and rows == [P, 0, 0, 0] and length == P and bool((parents == FILL).all())
    ar = torch.arange(P, dtype=torch.int32)
    assert torch.equal(maps[0, :P], ar) and torch.equal(maps[1, :P], ar) and bool((maps[2, :P] == -1).all()) and bool((maps[:, P:] == FILL).all())
    # k = 0 with clones: originals, then clones, no child entry
    sel, parents, rows, maps, length = _cabi_plan(F.get(F.MIXES[1]))
    assert sel == [P, P, 0, 0] and rows == [2 * P, 0, 0, 0] and length == 2 * P and bool((parents == FILL).all())
    assert torch.equal(maps[0, :2 * P], torch.cat([ar, ar])) and torch.equal(maps[1, :2 * P], torch.cat([ar, torch.full_like(ar, -1)]))
    assert bool((maps[2, :2 * P] == -1).all()) and bool((maps[:, 2 * P:] == FILL).all())
    # every child dropped: the kept rows in front, nothing behind them, the counts say where the children went
    sel, parents, rows, maps, length = _cabi_plan(F.get(F.MIXES[2]))
    assert sel == [P, 0, P - 5, 0] and rows == [5, 2 * (P - 5), 0, 0] and length == 5 + 2 * (P - 5)
    few = (torch.arange(5) * 60 + 3).to(torch.int32)
    assert torch.equal(maps[0, :5], few) and bool((maps[:, 5:] == FILL).all())
    assert torch.equal(parents[:P - 5], torch.tensor([i for i in range(P) if i not in few.tolist()], dtype=torch.int32)) and bool((parents[P - 5:] == FILL).all())


def test_cabi_empty_scene_writes_zero_counts():
    from _gsr import DensifyPlan, check, lib
    plan = DensifyPlan(F.MAX_GRAD, F.MIN_WEIGHT, 0.03, 0.3, 4.5, 9.0, (ctypes.c_float * 3)(0, 0, 0), 1, 2, 2)
    stream = torch.cuda.current_stream().cuda_stream
    for call in (lambda c: lib.gsr_densify_plan_select(0, ctypes.byref(plan), None, None, None, None, None, None, 0, c, None, stream),
                 lambda c: lib.gsr_densify_plan_rows(0, ctypes.byref(plan), None, 0, None, None, None, None, None, 0, None, None, None, c, stream),
                 lambda c: lib.gsr_prune_rows(0, None, None, 0, None, c, stream)):
        counts = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        check(call(counts.data_ptr()), "P = 0")
        assert counts.tolist() == [0, 0, 0, 0]


def test_cabi_scatter_rows_leaves_the_other_rows_alone():
    from _gsr import GatherGroup, check, lib
    g = torch.Generator().manual_seed(3)
    n, w = 1000, 3
    src = torch.randn(400, w, generator=g).cuda()
    dst0 = torch.randn(50 + n * w + 7, generator=g).cuda()
    slot = torch.where(torch.rand(n, generator=g) < 0.3, torch.randint(0, 400, (n,), generator=g), torch.full((n,), -1)).to(torch.int32).cuda()
    dst = dst0.clone()
    groups = (GatherGroup * 1)(GatherGroup(0, 50, w))
    check(lib.gsr_scatter_rows(src.data_ptr(), dst.data_ptr(), slot.data_ptr(), n, groups, 1, torch.cuda.current_stream().cuda_stream), "gsr_scatter_rows")
    want = dst0.clone()
    body = want[50:50 + n * w].view(n, w)
    body[slot >= 0] = src[slot[slot >= 0].long()]
    assert torch.equal(dst, want) and int((slot >= 0).sum()) > 100


# ------------------------------------------------------------------------------------------------- stream and scratch
def test_plan_on_a_side_stream_between_two_enqueued_kernels():
    """The statistics reach their buffer through a copy enqueued on the side stream behind a long kernel, and are overwritten right behind
    the call on that stream: a plan kernel on any other stream would read them too early or too late."""
    fx, st, want, _ = _both(F.MAIN, 20)
    staged = _stats(fx).buf.clone()
    filler = torch.zeros(64 << 20, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    from gsr_densify import DensifyStats
    with torch.cuda.stream(side):
        stats = DensifyStats(fx["P"], "cuda")
        for _ in range(4):
            filler.add_(1.0)
        stats.buf.copy_(staged)
        got = _run(fx, st, "device", 20, stats=stats)
        stats.buf.fill_(float("nan"))
        filler.add_(1.0)
    side.synchronize()
    _assert_same(got, want)


@pytest.mark.parametrize("pattern", [0xFF, 0x01])
def test_plan_does_not_depend_on_what_scratch_maps_and_counts_held(pattern):
    import poison
    fx, st, want, _ = _both(F.MAIN, 20)
    with poison.poisoned(pattern) as state:
        got = _run(fx, st, "device", 20)
    assert state.count >= 6          # scratch, both count buffers, the parents, the maps, the children
    _assert_same(got, want)


def test_host_reads_on_the_device_path():
    """One 16-byte read of the select counts; a second one of the kept count only with a size threshold; nothing else waits for the device."""
    fx = F.get(F.MAIN)
    st, stats, noise = _state(fx), _stats(fx), torch.from_numpy(_noise(fx)).cuda()
    from gsr_densify import densify_and_prune
    mean = torch.tensor(fx["mean"])
    torch.cuda.synchronize()
    for screen, reads in ((None, 1), (20, 2)):
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                densify_and_prune(st, stats, F.MAX_GRAD, F.MIN_OPACITY, mean, fx["extent"], screen, noise=noise, plan="device")
            finally:
                torch.cuda.set_sync_debug_mode("default")
        syncs = [w for w in seen if "called a synchronizing" in str(w.message)]      # (torch's sync debug mode: one warning per host wait)
        assert any("debug mode" in str(w.message) for w in seen) or syncs, "torch's sync debug mode said nothing at all"
        print("max_screen_size", screen, "host synchronisations:", len(syncs))
        assert len(syncs) == reads, [str(w.message) for w in syncs]


# ------------------------------------------------------------------------------------------------- sharded state
def test_sharded_state_world_2(monkeypatch):
    import gsr_densify
    world = 2
    fx = F.get(F.SHARDED)
    plain = _state(fx)
    shards = [_state(fx, shard=(r, world)) for r in range(world)]
    total, n = shards[0].params.total, shards[0].params.total // world
    pad = total - plain.params.total
    whole = [torch.cat([m, torch.zeros(pad, device="cuda")]) for m in (plain.optimizer.exp_avg, plain.optimizer.exp_avg_sq)]
    for r, s in enumerate(shards):
        s.optimizer.exp_avg.copy_(whole[0][r * n:(r + 1) * n])
        s.optimizer.exp_avg_sq.copy_(whole[1][r * n:(r + 1) * n])
    monkeypatch.setattr(gsr_densify, "_whole_moments", lambda state, group: (torch.cat([s.optimizer.exp_avg for s in shards]),
                                                                             torch.cat([s.optimizer.exp_avg_sq for s in shards])))
    for r, s in enumerate(shards):
        want, got = _run(fx, s, "torch", 20), _run(fx, s, "device", 20)
        _assert_same(got, want)
        assert got[0].shard == (r, world) and got[0].optimizer.exp_avg.numel() == got[0].params.total // world
        assert got[2]["split"] > 20 and got[2]["cloned"] > 20 and got[2]["pruned_big"] > 0


# ------------------------------------------------------------------------------------------------- prune_points
def _mask(P, seed=5):
    return torch.rand(P, generator=torch.Generator().manual_seed(seed)) < 0.3


def test_prune_points_equals_indexing_on_the_host():
    from gsr_densify import prune_points
    fx = F.get(F.SHARDED)
    P = fx["P"]
    st, stats = _state(fx), _stats(fx)
    st.optimizer.set_lr("opacities", 0.0123)
    mask = _mask(P)
    keep = ~mask
    new, new_stats, info = prune_points(st, mask.cuda(), stats)
    P1 = int(keep.sum())
    assert info == dict(pruned=P - P1, before=P, after=P1) and 0.25 * P < P - P1 < 0.35 * P
    for k in F.GROUPS:
        assert torch.equal(new.p[k].detach().cpu(), st.p[k].detach().cpu()[keep]), k
        for a, b in ((new.optimizer.exp_avg, st.optimizer.exp_avg), (new.optimizer.exp_avg_sq, st.optimizer.exp_avg_sq)):
            assert torch.equal(new.params.view_of(a, k).cpu(), st.params.view_of(b, k).cpu()[keep]), k
    assert new_stats.buf.shape == (5, P1) and torch.equal(new_stats.buf.cpu(), stats.buf.cpu()[:, keep])
    assert float(new_stats.buf.abs().max()) > 0
    for k in ("cubemap", "fail"):
        assert torch.equal(new.p[k].detach(), st.p[k].detach())
        assert torch.equal(new.params.view_of(new.optimizer.exp_avg, k), st.params.view_of(st.optimizer.exp_avg, k))
        assert torch.equal(new.params.view_of(new.optimizer.exp_avg_sq, k), st.params.view_of(st.optimizer.exp_avg_sq, k))
    o, n = st.optimizer, new.optimizer
    assert (n.step_count, n.betas, n.eps, n.groups) == (o.step_count, o.betas, o.eps, o.groups) == (17, (0.8, 0.99), 1e-8, o.groups)
    assert n.groups["opacities"][0] == 0.0123 and new.lrs == st.lrs and new.shard is None
    # the mask may live on the host; no statistics: none come back
    again, none, _ = prune_points(st, mask)
    assert none is None and torch.equal(again.params.flat, new.params.flat)
    # and the new state trains
    new.grads.flat.normal_()
    new.optimizer.step()
    assert torch.isfinite(new.params.flat).all()


def test_prune_points_with_an_all_false_mask_returns_equal_buffers():
    from gsr_densify import prune_points
    fx = F.get(F.SHARDED)
    st, stats = _state(fx), _stats(fx)
    new, new_stats, info = prune_points(st, torch.zeros(fx["P"], dtype=torch.bool, device="cuda"), stats)
    assert info == dict(pruned=0, before=fx["P"], after=fx["P"]) and new is not st
    assert torch.equal(new.params.flat, st.params.flat) and torch.equal(new_stats.buf, stats.buf)
    for k in st.params.names:          # (group by group: the padding between groups carries no moments)
        for a, b in ((new.optimizer.exp_avg, st.optimizer.exp_avg), (new.optimizer.exp_avg_sq, st.optimizer.exp_avg_sq)):
            assert torch.equal(new.params.view_of(a, k), st.params.view_of(b, k)), k


def test_prune_points_on_a_raw_train_state():
    from gsr_densify import prune_points
    from gsr_train import RawTrainState
    from poison import u32
    fx = F.get(F.SHARDED)
    st = _state(fx, raw=True)
    st.freeze(("means3D", "rotations"))
    mask = _mask(fx["P"], 6)
    new, _, info = prune_points(st, mask.cuda())
    assert type(new) is RawTrainState and new.optimizer.frozen == {"means3D", "rotations"} and info["after"] == int((~mask).sum())
    for k in F.GROUPS:
        assert torch.equal(new.p[k].detach().cpu(), st.p[k].detach().cpu()[~mask]), k
    for k in RawTrainState.ACTIVATED:           # the activated copy: gsr_activate of the raw rows = the old copy's rows
        assert torch.equal(new.a[k].detach().cpu(), st.a[k].detach().cpu()[~mask]), k
    have = new.optimizer.act.clone()
    new.optimizer.act.fill_(float("nan"))
    new.optimizer.activate()
    torch.cuda.synchronize()
    assert u32(have.cpu().numpy()).tobytes() == u32(new.optimizer.act.cpu().numpy()).tobytes()


def test_prune_points_refuses_a_bad_mask():
    from gsr_densify import prune_points
    fx = F.get(F.MIXES[0])
    st = _state(fx)
    P = fx["P"]
    for bad in (torch.zeros(P - 1, dtype=torch.bool), torch.zeros(P + 1, dtype=torch.bool, device="cuda"), torch.zeros(P, dtype=torch.uint8),
                torch.zeros(P, dtype=torch.float32), torch.zeros(P, 1, dtype=torch.bool), [False] * P, None):
        with pytest.raises(ValueError, match="mask"):
            prune_points(st, bad)
    from gsr_densify import DensifyStats
    with pytest.raises(ValueError, match="stats"):
        prune_points(st, torch.zeros(P, dtype=torch.bool), DensifyStats(P + 1, "cuda"))
    from gsr_densify import densify_and_prune
    with pytest.raises(ValueError, match="max_grad"):
        densify_and_prune(st, _stats(fx), 0.0, F.MIN_OPACITY, torch.tensor(fx["mean"]), fx["extent"], None, plan="device")
