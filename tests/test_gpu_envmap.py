"""gsr_envmap_resize / gsr_envmap_sharpen (include/gsr_hip_envmap.h) and the state transition around them (gsr_envmap.py) on the GPU, against
the float64 restatement of tests/envmap_ref.py (pinned against torch on the CPU by tests/test_envmap_ref.py).

Bounds (envmap_ref.RESIZE_REL_BOUND, envmap_ref.SHARPEN_ACT_BOUND) are worst-case derivations, not measurements:
  * resize: |out - ref| <= 4e-5 * max|src|.  Each weight is a degree-3 Horner form with intermediates up to 6 (a few tens of 2^-24), the
    fraction carries one rounding, each output sums 16 taps.  A wrong A (-0.5 moves outputs by about 3e-2), a wrong clamp or an off-by-one
    tap (O(1)) stay far outside.
  * sharpen, activated space: |sigmoid64(out) - ref_act| <= 4e-6 (float32 exp, a 10-term sum of values in [0, 1], a blend of magnitude at
    most 3); raw space: |out - ref_raw| <= 4e-6 / (o (1 - o)) + 1e-6 |ref_raw| with o the reference's activated value.
Every case prints the largest error it saw next to its bound."""
import math

import numpy as np
import pytest
import torch

import envmap_ref as E

pytestmark = pytest.mark.gpu

RESIZE_PAIRS = [(1, 2), (2, 4), (3, 6), (5, 9), (5, 10), (8, 16), (7, 3), (6, 6), (4, 1), (1, 1)]
RESIZE_CASES = [(p, a, b) for a, b in RESIZE_PAIRS for p in (6, 18)] + [(18, 128, 256)]
SHARPEN_SIZES = [1, 2, 3, 4, 5, 17, 128]
FACTORS = [0.0, 1.0, 2.0]
# |out| at the clamps: logit(fl32(1 - 1e-3)), whose argument is off by at most 2^-25 under a slope of 1001, and a few ulp of log(999) < 7
RAW_LIMIT = math.log(999.0) + 1001 * 2.0 ** -25 + 8 * 2.0 ** -24 * 7


def _rand(shape, seed, span=1.0):
    return ((torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * span).cuda()


def _resize(src, L_dst, dst=None):
    from _gsr import check, lib, stream_ptr
    planes, L_src = src.shape[0], src.shape[-1]
    if dst is None:
        dst = torch.full((planes, L_dst, L_dst), float("nan"), device=src.device)
    check(lib.gsr_envmap_resize(src.data_ptr(), dst.data_ptr(), planes, L_src, L_dst, stream_ptr(src.device)), "gsr_envmap_resize")
    return dst


def _sharpen(src, factor, dst=None, lo=E.LO, hi=E.HI):
    from _gsr import check, lib, stream_ptr
    planes, L = src.shape[0], src.shape[-1]
    if dst is None:
        dst = torch.full_like(src, float("nan"))
    check(lib.gsr_envmap_sharpen(src.data_ptr(), dst.data_ptr(), planes, L, factor, lo, hi, stream_ptr(src.device)), "gsr_envmap_sharpen")
    return dst


def _sharpen_texture(planes, L, seed):
    x = _rand((planes, L, L), seed, span=9.0)           # [-9, 9]: sigmoid goes below 1e-3 and above 1 - 1e-3
    x.view(-1)[0], x.view(-1)[-1] = -9.0, 9.0
    if L >= 3:
        x[0, 1, 1], x[-1, -2, -2] = 9.0, -9.0             # and an interior texel at each end
    return x


def _check_sharpen(out, x, factor, what):
    """out [.., L, L] float32 (CPU) against the restatement of x under both bounds; returns the two largest errors."""
    ref_act = E.sharpen_activated(x.double().numpy(), factor)
    ref_raw = np.log(ref_act / (1.0 - ref_act))
    got = out.double().numpy()
    assert np.isfinite(got).all() and np.abs(got).max() <= RAW_LIMIT, what
    err_act = np.abs(E.sigmoid(got) - ref_act)
    err_raw = np.abs(got - ref_raw)
    bound_raw = E.SHARPEN_ACT_BOUND / (ref_act * (1.0 - ref_act)) + 1e-6 * np.abs(ref_raw)
    print(f"{what}: activated {err_act.max():.3e} (bound {E.SHARPEN_ACT_BOUND:.0e}), raw / its bound {(err_raw / bound_raw).max():.3f}, "
          f"raw {err_raw.max():.3e}")
    assert (err_act <= E.SHARPEN_ACT_BOUND).all(), what
    assert (err_raw <= bound_raw).all(), what
    return float(err_act.max()), float(err_raw.max())


# ------------------------------------------------------------------------------------------------- the entries
@pytest.mark.parametrize("planes, L_src, L_dst", RESIZE_CASES, ids=lambda v: str(v))
def test_resize_matches_the_restatement_and_reproduces_coinciding_nodes(planes, L_src, L_dst):
    src = _rand((planes, L_src, L_src), 1000 * L_src + 10 * L_dst + planes)
    out = _resize(src, L_dst)
    torch.cuda.synchronize()
    s, o = src.cpu(), out.cpu()
    ref = E.resize(s.double().numpy(), L_dst)
    scale = float(s.abs().max())
    err = float(np.abs(o.double().numpy() - ref).max())
    print(f"resize {planes} x {L_src} -> {L_dst}: max error {err:.3e} = {err / scale:.3e} of max|src| (bound {E.RESIZE_REL_BOUND:.0e})")
    assert err <= E.RESIZE_REL_BOUND * scale
    # output nodes that lie on source nodes are those source texels: the four corners (of a single output node, all four are source node 0)
    a, b = [0, 0, -1, -1], [0, -1, 0, -1]
    far = -1 if L_dst > 1 else 0
    assert torch.equal(o[:, a, b], s[:, [0, 0, far, far], [0, far, 0, far]])
    if L_dst == L_src:
        assert torch.equal(o, s)
    if L_dst == 2 * L_src - 1:
        assert torch.equal(o[:, ::2, ::2], s)
    if L_src == 1:
        assert torch.equal(o, s.expand(planes, L_dst, L_dst))


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("planes", [6, 18])
@pytest.mark.parametrize("L", SHARPEN_SIZES)
def test_sharpen_matches_the_restatement_in_both_spaces(L, planes, factor):
    x = _sharpen_texture(planes, L, 31 * L + planes)
    out = _sharpen(x, factor)
    torch.cuda.synchronize()
    xc, oc = x.cpu(), out.cpu()
    _check_sharpen(oc, xc, factor, f"sharpen {planes} x {L}, factor {factor}")
    # border texels, and every texel of a plane of at most 2 x 2, are not sharpened: logit(clamp(sigmoid(x))) whatever the factor
    border = torch.ones(L, L, dtype=torch.bool)
    if L > 2:
        border[1:-1, 1:-1] = False
    plain = E.sharpen(xc.double().numpy(), 1.0)
    o = np.clip(E.sigmoid(xc.double().numpy()), E.LO, E.HI)
    bound = E.SHARPEN_ACT_BOUND / (o * (1.0 - o)) + 1e-6 * np.abs(plain)
    assert (np.abs(oc.double().numpy() - plain) <= bound)[:, border.numpy()].all()


@pytest.mark.parametrize("entry", ["resize", "sharpen"])
def test_every_element_of_dst_is_written_and_nothing_else(entry):
    planes, L, G = 18, 9, 4099
    n = planes * L * L
    buf = torch.full((G + n + G,), float("nan"), device="cuda")
    dst = buf[G:G + n].view(planes, L, L)
    if entry == "resize":
        _resize(_rand((planes, 5, 5), 5), L, dst=dst)
    else:
        _sharpen(_sharpen_texture(planes, L, 6), 2.0, dst=dst)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dst).all())
    assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all())


@pytest.mark.parametrize("entry", ["resize", "sharpen"])
def test_the_entries_run_on_the_callers_stream(entry):
    """On a side stream, behind work of that stream that writes src, with no host synchronisation in between: the result is the
    default-stream result."""
    planes, L = 18, 128
    values = _sharpen_texture(planes, L, 77)
    run = (lambda s, d=None: _resize(s, 2 * L, dst=d)) if entry == "resize" else (lambda s, d=None: _sharpen(s, 2.0, dst=d))
    want = run(values)
    torch.cuda.synchronize()
    src = torch.zeros_like(values)
    dst = torch.full_like(want, float("nan"))
    junk = torch.full((1024, 1024), 1.0 / 1024, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(16):
            junk = junk @ junk                             # (stays at 1 / 1024: the last product gates the copy below)
        src.copy_(values * (junk[0, 0] * 1024))
        run(src, dst)
    side.synchronize()
    assert torch.equal(dst, want)


# ------------------------------------------------------------------------------------------------- the state transition
P, M, L, C = 67, 16, 4, 3
SHAPES = dict(means3D=(P, 3), shs=(P, M, 3), opacities=(P, 1), scales=(P, 2), rotations=(P, 4), refl_strengths=(P, 1), cubemap=(6, C, L, L), fail=(C,))


def _state(kind, names=tuple(SHAPES), **kw):
    """A state of three Adam steps on seeded random gradients (non-zero moments everywhere), a fourth gradient left in the buffer, the
    scheduled position rate set.  Two calls give bit-identical states: the fused Adam is elementwise."""
    from gsr_train import GaussianTrainState, RawTrainState
    g = torch.Generator().manual_seed(2024)
    tensors = {k: torch.randn(SHAPES[k], generator=g) * 0.5 for k in names}
    st = (RawTrainState if kind == "raw" else GaussianTrainState)(tensors, "cuda", spatial_lr_scale=1.7, lrs=dict(refl_lr=0.004), **kw)
    st.update_learning_rate(1234)
    for i in range(4):
        st.grads.flat.copy_(torch.randn(st.params.total, generator=g))
        if i < 3:
            st.optimizer.step()
    return st


def _group_bits(st, k):
    """Parameters, gradient slot and both moments of group k, as CPU tensors."""
    a, b = st.params.slices[k]
    return [t[a:b].detach().cpu().clone() for t in (st.params.flat, st.grads.flat, st.optimizer.exp_avg, st.optimizer.exp_avg_sq)]


@pytest.mark.parametrize("kind", ["flat", "raw"])
def test_double_env_map_hands_the_state_over(kind):
    import gsr_envmap
    from gsr_train import RawTrainState
    old, twin = _state(kind), _state(kind)
    assert torch.equal(old.params.flat, twin.params.flat) and torch.equal(old.optimizer.exp_avg_sq, twin.optimizer.exp_avg_sq)
    if kind == "raw":
        for st in (old, twin):
            st.freeze(("means3D", "rotations"))
            st.optimizer.act.add_(0.125)                   # values that are not act(raw), as from_activated may leave them
    before = {k: _group_bits(old, k) for k in old.params.names}
    act_before = old.optimizer.act.cpu().clone() if kind == "raw" else None
    new = gsr_envmap.double_env_map(old)
    torch.cuda.synchronize()
    assert type(new) is type(old) and new is not old
    assert new.params.names == old.params.names
    assert new.params.shapes == dict(old.params.shapes, cubemap=(6, C, 2 * L, 2 * L))
    assert new.params.slices["fail"][0] > old.params.slices["fail"][0]                  # `fail` has moved
    for k in new.params.names:
        got = _group_bits(new, k)
        if k != "cubemap":
            assert all(torch.equal(x, y) for x, y in zip(got, before[k])), k
            assert all(bool(x.abs().sum() > 0) for x in got), k                         # (the comparison is not one of zeros)
    tex, grad, avg, sq = _group_bits(new, "cubemap")
    src = before["cubemap"][0].view(6 * C, L, L)
    err = float(np.abs(tex.double().numpy().reshape(6 * C, 2 * L, 2 * L) - E.resize(src.double().numpy(), 2 * L)).max())
    print(f"{kind}: texture {L} -> {2 * L} max error {err:.3e} (bound {E.RESIZE_REL_BOUND * float(src.abs().max()):.3e})")
    assert err <= E.RESIZE_REL_BOUND * float(src.abs().max())
    assert tuple(new.p["cubemap"].shape) == (6, C, 2 * L, 2 * L) and torch.equal(new.p["cubemap"].detach().cpu().reshape(-1), tex)
    assert not grad.any() and not avg.any() and not sq.any()
    assert new.optimizer.step_count == old.optimizer.step_count == 3
    assert new.optimizer.groups == old.optimizer.groups and new.optimizer.groups["means3D"][0] == old.xyz_scheduler_args(1234)
    assert new.lrs == old.lrs and new.spatial_lr_scale == old.spatial_lr_scale == 1.7
    assert (new.optimizer.betas, new.optimizer.eps) == (old.optimizer.betas, old.optimizer.eps)
    for k in new.params.names:                                                          # the views are those of the new buffers
        assert new.p[k].grad.data_ptr() == new.grads.view(k).data_ptr()
    if kind == "raw":
        assert isinstance(new, RawTrainState) and new.optimizer.frozen == {"means3D", "rotations"}
        assert torch.equal(new.optimizer.act.cpu(), act_before)
        assert new.optimizer.act_slices == old.optimizer.act_slices
    # one step right after: the texture stays bit for bit, everything else steps as on the state that was never touched
    new.optimizer.step()
    twin.optimizer.step()
    torch.cuda.synchronize()
    assert torch.equal(_group_bits(new, "cubemap")[0], tex)
    for k in new.params.names:
        if k != "cubemap":
            assert all(torch.equal(x, y) for x, y in zip(_group_bits(new, k), _group_bits(twin, k))), k
            moved = not torch.equal(_group_bits(new, k)[0], before[k][0])
            assert moved == (not (kind == "raw" and k in ("means3D", "rotations"))), k    # (the step did step; the frozen groups stayed)
    if kind == "raw":
        assert torch.equal(new.optimizer.act, twin.optimizer.act)


@pytest.mark.parametrize("kind", ["flat", "raw"])
def test_resize_to_the_same_resolution_keeps_the_texels_and_zeroes_the_moments(kind):
    import gsr_envmap
    old = _state(kind)
    before = {k: _group_bits(old, k) for k in old.params.names}
    new = gsr_envmap.resize_env_map(old, L)
    torch.cuda.synchronize()
    assert new is not old and new.params.slices == old.params.slices
    for k in new.params.names:
        got = _group_bits(new, k)
        if k == "cubemap":
            assert torch.equal(got[0], before[k][0]) and not got[1].any() and not got[2].any() and not got[3].any()
        else:
            assert all(torch.equal(x, y) for x, y in zip(got, before[k])), k


@pytest.mark.parametrize("kind", ["flat", "raw"])
def test_filter_env_map_sharpens_in_place_and_zeroes_the_textures_moments(kind):
    import gsr_envmap
    st = _state(kind)
    with torch.no_grad():
        st.p["cubemap"].mul_(12.0)                         # logits that reach both clamps
    before = {k: _group_bits(st, k) for k in st.params.names}
    grads_before = st.grads.flat.cpu().clone()
    act_before = st.optimizer.act.cpu().clone() if kind == "raw" else None
    assert gsr_envmap.filter_env_map(st) is st
    torch.cuda.synchronize()
    tex, grad, avg, sq = _group_bits(st, "cubemap")
    _check_sharpen(tex.view(6 * C, L, L), before["cubemap"][0].view(6 * C, L, L), 2.0, f"{kind}: filter_env_map")
    assert not avg.any() and not sq.any()
    assert torch.equal(st.grads.flat.cpu(), grads_before)
    for k in st.params.names:
        if k != "cubemap":
            assert all(torch.equal(x, y) for x, y in zip(_group_bits(st, k), before[k])), k
    assert st.optimizer.step_count == 3
    if kind == "raw":
        assert torch.equal(st.optimizer.act.cpu(), act_before)
    other = gsr_envmap.filter_env_map(st, factor=1.0)      # factor 1: logit(clamp(sigmoid)) of what the first pass left, which is inside the clamps
    torch.cuda.synchronize()
    assert other is st
    _check_sharpen(_group_bits(st, "cubemap")[0].view(6 * C, L, L), tex.view(6 * C, L, L), 1.0, f"{kind}: filter_env_map(factor=1)")


def test_python_refusals():
    import gsr_envmap
    no_env = _state("flat", names=[k for k in SHAPES if k not in ("cubemap", "fail")])
    for call in (lambda s: gsr_envmap.resize_env_map(s, 8), gsr_envmap.double_env_map, gsr_envmap.filter_env_map):
        with pytest.raises(ValueError, match="cubemap"):
            call(no_env)
    st = _state("flat")
    for bad in (0, -1):
        with pytest.raises(ValueError, match="new_resolution"):
            gsr_envmap.resize_env_map(st, bad)
    from gsr_train import GaussianTrainState
    g = torch.Generator().manual_seed(1)
    sharded = GaussianTrainState({k: torch.randn(SHAPES[k], generator=g) for k in SHAPES}, "cuda", shard=(1, 2))
    for call in (lambda s: gsr_envmap.resize_env_map(s, 8), gsr_envmap.double_env_map, gsr_envmap.filter_env_map):
        with pytest.raises(NotImplementedError, match="sharded"):
            call(sharded)
    one_rank = GaussianTrainState({k: torch.randn(SHAPES[k], generator=g) for k in SHAPES}, "cuda", shard=(0, 1))
    assert gsr_envmap.double_env_map(one_rank).params.shapes["cubemap"] == (6, C, 2 * L, 2 * L)       # a single rank holds everything


def test_the_new_state_renders_its_environment_map():
    """gaussian_renderer.render_env_map on the new state's model at L = 8: finite, and the panorama of a CubemapEncoder that holds the new
    state's texture bit for bit (the same lookup kernel on the same values)."""
    import gsr_envmap
    from cubemapencoder import CubemapEncoder
    from gaussian_renderer import render_env_map
    new = gsr_envmap.double_env_map(_state("raw"))
    got = render_env_map(new.model(), height=32, width=64)
    enc = CubemapEncoder(output_dim=C, resolution=2 * L).cuda()
    with torch.no_grad():
        enc.set_textures(new.p["cubemap"].detach().clone())
        enc.params["Cubemap_failv"].copy_(new.p["fail"].detach())

    class Holder:
        get_envmap = enc
    want = render_env_map(Holder, height=32, width=64)
    torch.cuda.synchronize()
    for key in ("env_cood1", "env_cood2"):
        assert tuple(got[key].shape) == (3, 32, 64) and bool(torch.isfinite(got[key]).all())
        assert torch.equal(got[key], want[key])
