"""The env-scope pass on the GPU: utils.loss_utils.env_scope_masks / refl_scope_loss (gsr_env_scope_forward / _backward,
include/gsr_hip_scope.h), GaussianTrainState.refl_scope_loss, RawTrainState.dist_color and render()'s pipe.gsr_env_scope_mask, against
tests/env_scope_ref.py, the float64 restatement pinned to the reference's torch expressions in tests/test_env_scope_ref.py.

Masks are compared for EQUALITY: every point set used here keeps clear of the band in which a float32 evaluation may fall on either
side of the sphere (env_scope_ref.band), or sits exactly on it (the lattice), so every correct evaluation gives the same masks.

The bound of the sum.  The forward kernel runs min(1024, ceil(P / 256)) blocks of 256 threads, one point per thread per trip of its
grid-stride loop.  A term reaches the float32 result through
    T = ceil(P / (256 * blocks))   additions in its thread's accumulator (the first one, to 0, is exact and pays for the double sum's own error),
    6                              wave steps (row_shr 1, 2, 4, 8, row_bcast 15, 31),
    2                              block steps ((w0 + w1) + (w2 + w3)),
    1                              rounding of the double sum of the block pairs to float32,
so d = T + 9 and |S - S64| <= d * 2^-24 * sum over the outside rows of |refl| (`sum_depth`).  The count takes the same path with exact additions."""
import math

import numpy as np
import pytest
import torch

import env_scope_ref as E
import raw_step_ref as R
from poison import PATTERNS, poisoned, u32

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
BLOCK_CAP = 1024
P_TWO_TRIPS = 2 * BLOCK_CAP * 256 + 77       # the grid-stride loop runs three times for the first 77 threads and ends in a partial block
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, P_TWO_TRIPS)
_cache = {}


def sum_depth(P):
    blocks = min(BLOCK_CAP, (P + 255) // 256)
    return math.ceil(P / (256 * blocks)) + 9


def points(kind, P):
    """The point set and its float64 masks, made once per (kind, P) and never modified."""
    key = (kind, P)
    if key not in _cache:
        if kind == "clear":
            xyz, refl, c, r = E.clear_points(P, seed=P)
        elif kind == "shell":
            xyz, refl, c, r = E.shell_points(P, seed=P)[:4]
        else:
            xyz, refl, c, r = E.lattice_points()[:4]
        assert not (E.band(xyz, c, r) & (E.d2(xyz, c) != E.radius2(r))).any()
        inside, outside = E.masks(xyz, c, r)
        for a in (xyz, refl, inside, outside):
            a.setflags(write=False)
        _cache[key] = (xyz, refl, c, r, inside, outside)
    return _cache[key]


def dev(a, **kw):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(kw.get("grad", False))


def bits(t):
    return u32(t.detach().cpu().numpy()).tobytes()


def torch_masks(x, c, r):
    """The reference's float32 expressions on the device (render()'s and train.py's)."""
    centre = torch.tensor([float(v) for v in c], device=x.device)
    d2 = torch.sum((x - centre[None]) ** 2, dim=-1)
    return d2 < r ** 2, d2 > r ** 2


# ------------------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("kind", ["clear", "shell"])
def test_masks_equal_the_float64_restatement(kind, P):
    from utils.loss_utils import env_scope_masks, refl_scope_loss
    assert int(_lib().gsr_env_scope_scratch_floats()) == 2 * BLOCK_CAP
    xyz, refl, c, r, inside, outside = points(kind, P)
    x = dev(xyz)
    mi, mo = env_scope_masks(x, c, r)
    loss, li, lo = refl_scope_loss(dev(refl), x, c, r)
    ti, to = torch_masks(x, c, r)
    torch.cuda.synchronize()
    assert mi.dtype == torch.bool and mo.dtype == torch.bool and mi.shape == (P,) and mo.shape == (P,)
    print(f"{kind} P={P}: inside {int(mi.sum())} outside {int(mo.sum())}; bitwise equal to torch's float32 expressions on the device: "
          f"{bool(torch.equal(mi, ti) and torch.equal(mo, to))}")
    assert (mi.cpu().numpy() == inside).all() and (mo.cpu().numpy() == outside).all()
    assert not bool((mi & mo).any())
    assert torch.equal(li, mi) and torch.equal(lo, mo)                      # masks-only and loss calls
    assert set(np.unique(mi.view(torch.uint8).cpu().numpy())) <= {0, 1} and set(np.unique(mo.view(torch.uint8).cpu().numpy())) <= {0, 1}


def test_lattice_points_on_the_sphere_nan_and_inf():
    from utils.loss_utils import env_scope_masks, refl_scope_loss
    xyz, refl, c, r, want_in, want_out = E.lattice_points()
    x = dev(xyz)
    mi, mo = env_scope_masks(x, c, r)
    loss, li, lo = refl_scope_loss(dev(refl), x, c, r)
    ti, to = torch_masks(x, c, r)
    torch.cuda.synchronize()
    print("lattice: bitwise equal to torch's float32 expressions on the device:", bool(torch.equal(mi, ti) and torch.equal(mo, to)))
    assert (mi.cpu().numpy() == want_in).all() and (mo.cpu().numpy() == want_out).all()
    assert torch.equal(li, mi) and torch.equal(lo, mo) and not bool((mi & mo).any())
    s, n, mean = E.loss(refl, want_out)
    assert n == 2 and abs(float(loss.detach()) - mean) <= np.spacing(np.float32(mean)) + sum_depth(8) * E.U * s / n      # the NaN row's refl is not summed


# ------------------------------------------------------------------------------------------------------------ sums and loss
def _lib():
    import _gsr
    return _gsr.lib


def _forward(xyz, refl, c, r):
    """(inside, outside, sums) of one gsr_env_scope_forward call through the package's own marshaling."""
    from utils import loss_utils as lu
    return lu._scope_forward(dev(xyz), dev(refl), lu._scope_sphere(c, r))


@pytest.mark.parametrize("P", [1, 257, 1000, 4097, P_TWO_TRIPS])
def test_sums_count_and_loss(P):
    from utils.loss_utils import refl_scope_loss
    xyz, refl, c, r, inside, outside = points("clear", P)
    _, mo, sums = _forward(xyz, refl, c, r)
    _, _, again = _forward(xyz, refl, c, r)
    loss = refl_scope_loss(dev(refl), dev(xyz), c, r)[0]
    torch.cuda.synchronize()
    s64, n, mean = E.loss(refl, outside)
    got = sums.cpu().numpy().astype(np.float64)
    bound = sum_depth(P) * E.U * float(np.abs(refl.astype(np.float64))[outside].sum())
    print(f"P={P}: count {n}, |S - S64| = {abs(got[0] - s64):.3e} (bound {bound:.3e}, d = {sum_depth(P)}), loss {float(loss.detach()):.9g} against {mean:.9g}")
    assert got[1] == n
    assert bits(sums) == bits(again)
    if n == 0:
        assert got[0] == 0 and math.isnan(float(loss.detach()))
        return
    assert abs(got[0] - s64) <= bound
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert abs(float(loss.detach()) - mean) <= bound / n + np.spacing(np.float32(mean))


def test_all_points_outside_and_no_point_outside():
    from utils.loss_utils import refl_scope_loss
    xyz, refl, _, _, _, _ = points("clear", 1000)
    far = (100.0, 100.0, 100.0)
    # all outside
    r1 = dev(refl, grad=True)
    loss, mi, mo = refl_scope_loss(r1, dev(xyz), far, 1.0)
    loss.backward()
    torch.cuda.synchronize()
    s64 = float(refl.astype(np.float64).sum())
    assert bool(mo.all()) and not bool(mi.any())
    assert abs(float(loss.detach()) - s64 / 1000) <= sum_depth(1000) * E.U * s64 / 1000 + np.spacing(np.float32(s64 / 1000))
    assert np.abs(r1.grad.cpu().numpy().astype(np.float64) - 1e-3).max() <= 2 * np.spacing(np.float32(1e-3))
    # none outside: NaN value, no gradient to any row, and never a NaN in a gradient
    r2 = dev(refl, grad=True)
    loss, mi, mo = refl_scope_loss(r2, dev(xyz), far, 1000.0)
    loss.backward()
    assert math.isnan(float(loss.detach())) and bool(mi.all()) and not bool(mo.any())
    assert bits(r2.grad) == bits(torch.zeros(1000))
    for accumulate in (False, True):
        sink = torch.full((1000,), float("nan"), device="cuda") if not accumulate else dev(np.linspace(-1, 1, 1000).astype(np.float32))
        before = sink.clone()
        r3 = dev(refl, grad=True)
        loss = refl_scope_loss(r3, dev(xyz), far, 1000.0, grad_sink=sink, accumulate=accumulate)[0]
        (0.4 * loss).backward()
        torch.cuda.synchronize()
        assert r3.grad is None
        assert bits(sink) == (bits(before) if accumulate else bits(torch.zeros(1000)))


def test_empty_scene():
    from utils.loss_utils import env_scope_masks, refl_scope_loss
    x = torch.zeros(0, 3, device="cuda")
    mi, mo = env_scope_masks(x, (0, 0, 0), 1.0)
    assert mi.shape == (0,) and mo.shape == (0,) and mi.dtype == torch.bool
    refl = torch.zeros(0, 1, device="cuda", requires_grad=True)
    with poisoned(0xFF):                                   # sums must be WRITTEN (0, 0), not left as they were
        loss, li, lo = refl_scope_loss(refl, x, (0, 0, 0), 1.0)
    loss.backward()
    torch.cuda.synchronize()
    assert math.isnan(float(loss.detach())) and li.shape == (0,) and refl.grad.shape == (0, 1)
    from utils import loss_utils as lu
    with poisoned(0x01):
        sums = lu._scope_forward(x, torch.zeros(0, device="cuda"), lu._scope_sphere((0, 0, 0), 1.0))[2]
    assert bits(sums) == bits(torch.zeros(2))


# ------------------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize("P", [257, 4097])
def test_gradient_under_plain_autograd(P):
    from utils.loss_utils import refl_scope_loss
    xyz, refl, c, r, inside, outside = points("clear", P)
    n = int(outside.sum())
    x = dev(xyz)

    def check(grad, g, what):
        got = grad.cpu().numpy().reshape(-1).astype(np.float64)
        want = E.gradient(outside, g)
        assert (got[~outside] == 0).all(), what
        err = np.abs(got[outside] - want[outside]).max()
        print(f"P={P} {what}: upstream {g:.9g}, largest error on outside rows {err:.3e} (g / count = {g / n:.3e})")
        assert err <= 2 * np.spacing(np.float32(abs(g) / n)), what

    for factor in (1.0, 0.4):
        leaf = dev(refl[:, None], grad=True)
        loss, mi, mo = refl_scope_loss(leaf, x, c, r)
        assert not mi.requires_grad and not mo.requires_grad and loss.requires_grad
        (factor * loss).backward()
        assert leaf.grad.shape == (P, 1)
        check(leaf.grad, factor, f"factor {factor}")
    # an upstream gradient that a larger graph computes on the device; xyz asks for a gradient and gets none, as in the reference
    leaf, x = dev(refl, grad=True), dev(xyz, grad=True)
    w = dev(np.linspace(0.5, 1.5, 7).astype(np.float32), grad=True)
    loss = refl_scope_loss(leaf, x, c, r)[0]
    k = (w ** 2).sum()
    (loss * k).backward()
    torch.cuda.synchronize()
    check(leaf.grad, float(k.detach()), "upstream from a larger graph")
    w3 = float(w.detach()[3])
    assert abs(float(w.grad[3]) - 2 * w3 * float(loss.detach())) <= 4 * ULP * abs(2 * w3 * float(loss.detach()))
    assert x.grad is None


@pytest.mark.parametrize("P", [257, 4097])
def test_gradient_sink_accumulates_on_outside_rows_only(P):
    from utils.loss_utils import refl_scope_loss
    xyz, refl, c, r, inside, outside = points("clear", P)
    n = int(outside.sum())
    seeded = np.random.RandomState(P).uniform(0.5, 1.5, (P, 1)).astype(np.float32)       # positive: the sum is no smaller than either term
    sink = dev(seeded).clone()
    before = sink.clone()
    leaf = dev(refl[:, None], grad=True)
    loss = refl_scope_loss(leaf, dev(xyz), c, r, grad_sink=sink, accumulate=True)[0]
    (0.4 * loss).backward()
    torch.cuda.synchronize()
    assert leaf.grad is None
    got, was = sink.cpu().numpy().reshape(-1), before.cpu().numpy().reshape(-1)
    assert u32(got[~outside]).tobytes() == u32(was[~outside]).tobytes()
    want = was[outside].astype(np.float64) + 0.4 / n
    assert (np.abs(got[outside].astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all()
    assert (got[outside] != was[outside]).all()
    with pytest.raises(ValueError):
        refl_scope_loss(leaf, dev(xyz), c, r, accumulate=True)
    with pytest.raises(ValueError):
        refl_scope_loss(leaf, dev(xyz), c, r, grad_sink=torch.zeros(P, device="cuda"))       # refl is [P,1]


def test_no_result_depends_on_what_the_buffers_held():
    """accumulate=False overwrites the whole sink; masks, sums and scratch come from torch.empty: every pattern of tests/poison.py in all of
    them gives the same bits."""
    from utils.loss_utils import env_scope_masks, refl_scope_loss
    P = 4097
    xyz, refl, c, r, inside, outside = points("clear", P)
    results = []
    for pattern in PATTERNS:
        sink = torch.empty(P, device="cuda")
        sink.view(torch.uint8).fill_(pattern)
        leaf = dev(refl, grad=True)
        with poisoned(pattern) as state:
            loss, mi, mo = refl_scope_loss(leaf, dev(xyz), c, r, grad_sink=sink, accumulate=False)
            (0.4 * loss).backward()
            oi, oo = env_scope_masks(dev(xyz), c, r)
            plain = dev(refl, grad=True)
            refl_scope_loss(plain, dev(xyz), c, r)[0].backward()
        torch.cuda.synchronize()
        assert state.count >= 4
        results.append(tuple(bits(t) for t in (loss, mi.view(torch.uint8), mo.view(torch.uint8), sink, oi.view(torch.uint8), oo.view(torch.uint8),
                                               plain.grad)))
        want = E.gradient(outside, 0.4)
        got = sink.cpu().numpy().astype(np.float64)
        assert (got[~outside] == 0).all() and np.abs(got - want).max() <= 2 * np.spacing(np.float32(0.4 / outside.sum()))
    assert results[0] == results[1] == results[2]


# ------------------------------------------------------------------------------------------------------------ layouts and streams
def test_layouts_and_dtypes():
    from utils.loss_utils import env_scope_masks, refl_scope_loss
    P = 1000
    xyz, refl, c, r, inside, outside = points("clear", P)
    ref_i, ref_o = env_scope_masks(dev(xyz), c, r)
    ref_leaf = dev(refl, grad=True)
    ref_loss = refl_scope_loss(ref_leaf, dev(xyz), c, r)[0]
    ref_loss.backward()
    # a non-contiguous view
    wide = torch.full((P, 5), float("nan"), device="cuda")
    wide[:, 1:4] = dev(xyz)
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    # float64 coordinates that round to the float32 ones (the restatement reads the float32 coordinates)
    x64 = dev(xyz).double() + 1e-9 * dev(xyz).double()
    assert torch.equal(x64.float(), dev(xyz))
    # the centre as a tensor
    for x, centre in ((view, c), (x64, c), (dev(xyz), torch.tensor(c)), (dev(xyz), torch.tensor(c, dtype=torch.float64, device="cuda"))):
        mi, mo = env_scope_masks(x, centre, r)
        assert torch.equal(mi, ref_i) and torch.equal(mo, ref_o)
    for shape, dtype in (((P, 1), torch.float32), ((P,), torch.float64), ((P, 1), torch.float64)):
        leaf = dev(refl).to(dtype).reshape(shape).requires_grad_(True)
        loss, mi, mo = refl_scope_loss(leaf, view, c, r)
        loss.backward()
        assert leaf.grad.shape == shape and leaf.grad.dtype == dtype
        assert bits(loss) == bits(ref_loss) and torch.equal(mo, ref_o)
        assert bits(leaf.grad.float().reshape(-1)) == bits(ref_leaf.grad)
    strided = torch.zeros(P, 2, device="cuda")
    strided[:, 0] = dev(refl)
    leaf = strided.requires_grad_(True)
    loss = refl_scope_loss(leaf[:, 0], dev(xyz), c, r)[0]
    loss.backward()
    assert bits(loss) == bits(ref_loss) and bits(leaf.grad[:, 0].contiguous()) == bits(ref_leaf.grad) and not bool(leaf.grad[:, 1].any())
    with pytest.raises(ValueError):
        env_scope_masks(dev(xyz)[:, :2], c, r)
    with pytest.raises(ValueError):
        refl_scope_loss(dev(refl)[:-1], dev(xyz), c, r)
    with pytest.raises(RuntimeError):
        env_scope_masks(torch.from_numpy(np.array(xyz)), c, r)               # not on the device


def test_on_a_side_stream_with_late_inputs():
    """In the manner of tests/test_gpu_streams.py: the inputs hold NaN until a delay on the side stream has run out; forward and backward
    issued under that stream must come out as on the default stream.  The control first: an op issued on the DEFAULT stream without an
    event reads the poison, so the two streams do run side by side."""
    import stream_probe as SP
    from utils.loss_utils import refl_scope_loss
    P, delay = 4097, 20.0
    xyz, refl, c, r, inside, outside = points("clear", P)
    leaf = dev(refl, grad=True)
    ref_sink = torch.zeros(P, device="cuda")
    ref_loss, ref_i, ref_o = refl_scope_loss(leaf, dev(xyz), c, r, grad_sink=ref_sink)
    (0.4 * ref_loss).backward()
    torch.cuda.synchronize()
    default, side, tried = torch.cuda.default_stream(), None, 0
    while side is None and tried < 8:
        cand = torch.cuda.Stream()
        tried += 1
        with torch.cuda.stream(cand):
            torch.ones(4096, device="cuda") * 2
        torch.cuda.synchronize()
        late = SP.late_inputs(cand, {"x": np.ones(4096, np.float32)}, ms=delay)["x"]
        unordered = SP.fetch(default, {"y": late * 2})["y"]
        torch.cuda.synchronize()
        if not np.isfinite(unordered).all():
            side = cand
    if side is None:
        # as tests/test_gpu_streams.py's control: behind streams that serialise the test would pass whatever the library did
        raise RuntimeError("stream test: the %g ms delay (%.0f sleep cycles per ms) held the late inputs back on none of %d candidate "
                           "streams: no unordered read on the default stream came back as poison" % (delay, SP.cycles_per_ms(), tried))
    late = SP.late_inputs(side, {"xyz": np.array(xyz), "refl": np.array(refl)}, ms=delay)
    with torch.cuda.stream(side):
        sink = torch.full((P,), float("nan"), device="cuda")
        leaf = late["refl"].requires_grad_(True)
        loss, mi, mo = refl_scope_loss(leaf, late["xyz"], c, r, grad_sink=sink)
        (0.4 * loss).backward()
    got = SP.fetch(side, {"loss": loss.detach(), "inside": mi, "outside": mo, "sink": sink})
    torch.cuda.synchronize()
    ref = {"loss": ref_loss.detach(), "inside": ref_i, "outside": ref_o, "sink": ref_sink}
    for k in got:
        assert SP.same_bits(got[k], ref[k].cpu().numpy()), k


def test_no_host_synchronisation():
    from utils.loss_utils import refl_scope_loss
    P = 4097
    xyz, refl, c, r, inside, outside = points("clear", P)
    x, leaf, ref_leaf = dev(xyz), dev(refl[:, None], grad=True), dev(refl[:, None], grad=True)
    sink = torch.zeros(P, 1, device="cuda")
    refl_scope_loss(leaf, x, c, r)[0].backward()           # (first launches, first allocations)
    centre = torch.tensor([float(v) for v in c], device="cuda")
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as ex:                                 # noqa: BLE001
        pytest.skip(f"this build rejects torch.cuda.set_sync_debug_mode('error'): {ex}")
    try:
        loss, mi, mo = refl_scope_loss(leaf, x, list(c), r)
        (0.4 * loss).backward()
        loss2 = refl_scope_loss(leaf, x, c, r, grad_sink=sink, accumulate=True)[0]
        (0.4 * loss2).backward()
        with pytest.raises(RuntimeError):                   # the reference's expression does wait for the device: the mode works here
            msk = torch.sum((x - centre[None]) ** 2, dim=-1) > r ** 2
            ref_leaf[msk].mean().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(sink.any())


# ------------------------------------------------------------------------------------------------------------ state level
SP_, SW, SH, SL = 5000, 160, 120, 16        # the scene and sizes of tests/test_gpu_raw_train.py
NAMES = ["means3D", "shs", "opacities", "scales", "rotations", "refl_strengths"]
ZERO_LRS = dict(position_lr_init=0.0, position_lr_final=0.0, feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0, rotation_lr=0.0, refl_lr=0.0,
                envmap_cubemap_lr=0.0)


def _scene(seed=9, mu=-2.6):
    import gsr_synth as S
    if "scene" not in _cache:
        sc = S.make_scene(SP_, "S", seed=seed, mu=mu)
        tex, fail = S.make_cubemap(SL, 3, seed)
        cam = S.make_camera(SW, SH)
        act = {k: torch.from_numpy(sc[k]) for k in NAMES}
        act["cubemap"], act["fail"] = torch.from_numpy(tex), torch.from_numpy(fail)
        # a sphere about the median point through the widest gap between neighbouring distances near their median: about half of the
        # points outside, none in the ambiguous band
        xyz = sc["means3D"].astype(np.float32)
        c = tuple(float(v) for v in np.median(xyz, axis=0))
        d = np.sort(np.sqrt(E.d2(xyz, c)))
        k = SP_ // 2 - 50 + int(np.argmax(np.diff(d[SP_ // 2 - 50:SP_ // 2 + 50])))
        r = float(0.5 * (d[k] + d[k + 1]))
        assert not E.band(xyz, c, r).any()
        _cache["scene"] = (sc, act, cam, c, r)
    sc, act, cam, c, r = _cache["scene"]
    ct = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cam.items() if isinstance(v, np.ndarray)}
    return sc, act, cam, ct, c, r


def test_state_loss_alone_reaches_the_raw_gradient_through_the_step():
    from gsr_train import RawTrainState
    sc, act, cam, ct, c, r = _scene()
    st = RawTrainState.from_activated(act, "cuda", lrs=ZERO_LRS)
    st.optimizer.activate()
    raw0 = st.params.flat.clone()
    st.grads.flat.fill_(float("nan"))
    st.grads.zero_()
    st.grads.view("refl_strengths").fill_(float("nan"))        # accumulate=False overwrites the slot
    value, inside, outside = st.refl_scope_loss(c, r, weight=0.4, accumulate=False)
    st.update_learning_rate(1)
    st.set_lr("means3D", 0.0)
    st.optimizer.step()
    torch.cuda.synchronize()
    want_i, want_o = E.masks(sc["means3D"], c, r)
    out = outside.cpu().numpy()
    assert (out == want_o).all() and (inside.cpu().numpy() == want_i).all()
    n = int(out.sum())
    assert 0.3 * SP_ < n < 0.7 * SP_
    assert bits(st.params.flat) == bits(raw0)
    a, b = st.params.slices["refl_strengths"]
    raw = raw0[a:b].cpu().numpy().astype(np.float64)
    act64 = R.activation(R.ACTIVATED["refl_strengths"], raw)
    s64, _, mean = E.loss(act64.astype(np.float32), out)
    assert not value.requires_grad and abs(float(value) - 0.4 * mean) <= 4 * ULP * 0.4 * mean + sum_depth(SP_) * E.U * 0.4 * mean
    want = R.raw_gradient(R.ACTIVATED["refl_strengths"], raw, E.gradient(out, 0.4))
    got = st.optimizer.exp_avg.cpu().numpy().astype(np.float64) / (1.0 - R.f32(0.9))
    # torch's float32 chain on the same raw values: sigmoid, boolean index, mean, backward
    leaf = raw0[a:b].clone().requires_grad_(True)
    (0.4 * torch.sigmoid(leaf)[outside].mean()).backward()
    e32 = float(np.abs(leaf.grad.cpu().numpy().astype(np.float64) - want).max())
    err, scale = float(np.abs(got[a:b] - want).max()), float(np.abs(want).max())
    print(f"raw gradient of refl_strengths: device {err:.3e}, torch float32 chain {e32:.3e}, largest {scale:.3e}, count {n}")
    assert scale > 0 and err <= 4 * e32 + 2 * ULP * scale
    assert (got[a:b][~out] == 0).all()
    m, v = st.optimizer.exp_avg.clone(), st.optimizer.exp_avg_sq.clone()
    m[a:b] = 0
    v[a:b] = 0
    assert not bool(m.any()) and not bool(v.any())


def _rasterizer(cam, ct):
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    return GaussianRasterizer(GaussianRasterizationSettings(image_height=SH, image_width=SW, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                                            bg=torch.zeros(3, device="cuda"), scale_modifier=1.0, viewmatrix=ct["viewmatrix"],
                                                            projmatrix=ct["projmatrix"], sh_degree=3, campos=ct["campos"], prefiltered=False, debug=False))


@pytest.mark.parametrize("state", ["raw", "activated"])
def test_state_loss_adds_to_what_the_rasterizer_left_in_the_sink(state):
    from gaussian_renderer import deferred_reflection
    from gsr_train import GaussianTrainState, RawTrainState
    from utils.loss_utils import photometric_loss
    sc, act, cam, ct, c, r = _scene()
    st = RawTrainState.from_activated(act, "cuda", lrs=ZERO_LRS) if state == "raw" else GaussianTrainState(act, "cuda", lrs=ZERO_LRS)
    x = st.render_inputs() if state == "raw" else st.p
    gt = torch.rand(3, SH, SW, generator=torch.Generator().manual_seed(5)).cuda()
    rast = _rasterizer(cam, ct)
    sink = st.grads.sink()
    rast.set_grad_sink(sink)
    st.grads.zero_except_(sink)

    class Env:
        params = {"Cubemap_texture": x["cubemap"], "Cubemap_failv": x["fail"]}
    means2D = torch.zeros(SP_, 3, device="cuda", requires_grad=True)
    base, radii, allmap, refl_map, gw = rast(means3D=x["means3D"], means2D=means2D, opacities=x["opacities"], shs=x["shs"],
                                             refl_strengths=x["refl_strengths"], scales=x["scales"], rotations=x["rotations"],
                                             env_scope_mask=torch.from_numpy(sc["env_scope_mask"]).cuda())
    final, _, _ = deferred_reflection(allmap[2:5], base, refl_map, Env, ct["viewmatrix"], (SH, SW, cam["K"]), ct["R"], ct["T"])
    photometric_loss(final, gt, 0.2).backward()
    torch.cuda.synchronize()
    before = st.grads.flat.clone()
    assert bool(st.grads.view("refl_strengths").any())
    value, inside, outside = st.refl_scope_loss(c, r)           # weight 0.4, accumulate=True
    torch.cuda.synchronize()
    out = outside.cpu().numpy()
    n = int(out.sum())
    assert (out == E.masks(sc["means3D"], c, r)[1]).all() and n > 0
    a, b = st.params.slices["refl_strengths"]
    got, was = st.grads.flat.cpu().numpy(), before.cpu().numpy()
    keep = np.ones(got.shape[0], dtype=bool)
    keep[a:b] = ~out
    assert u32(got[keep]).tobytes() == u32(was[keep]).tobytes()
    want = was[a:b][out].astype(np.float64) + 0.4 / n
    # what the rasterizer left has either sign, so the sum may be smaller than the term added and "1 ulp of the sum" does not cover the
    # term's own roundings (float32(0.4), then the division: 1 ulp of 0.4 / n together); the addition rounds by half an ulp of the sum
    new = got[a:b][out]
    half_ulp_of_sum = 0.5 * np.maximum(np.spacing(np.abs(want).astype(np.float32)), np.spacing(np.abs(new)))
    assert (np.abs(new.astype(np.float64) - want) <= half_ulp_of_sum + np.spacing(np.float32(0.4 / n))).all()
    refl = (st.a if state == "raw" else st.p)["refl_strengths"].detach().cpu().numpy().reshape(-1)
    mean = E.loss(refl, out)[2]
    assert abs(float(value) - 0.4 * mean) <= 4 * ULP * 0.4 * mean + sum_depth(SP_) * E.U * 0.4 * mean


def test_state_loss_refuses_a_sharded_state():
    """Every rank would add the whole term and the reduce-scatter would sum it world_size times: refused before anything is written."""
    from gsr_train import GaussianTrainState
    sc, act, cam, ct, c, r = _scene()
    st = GaussianTrainState(act, "cuda", lrs=ZERO_LRS, shard=(0, 2))
    st.grads.flat.fill_(0.25)
    with pytest.raises(NotImplementedError):
        st.refl_scope_loss(c, r)
    torch.cuda.synchronize()
    assert bool((st.grads.flat == 0.25).all())


def test_render_takes_the_mask_from_the_pipe():
    from gaussian_renderer import render
    from gsr_train import RawTrainState
    from utils.loss_utils import env_scope_masks
    sc, act, cam, ct, c, r = _scene()

    class View:
        FoVx, FoVy = 2 * np.arctan(cam["tanfovx"]), 2 * np.arctan(cam["tanfovy"])
        image_width, image_height = SW, SH
        world_view_transform, full_proj_transform, camera_center = ct["viewmatrix"], ct["projmatrix"], ct["campos"]
        HWK, R, T = (SH, SW, cam["K"]), ct["R"], ct["T"]
        znear, zfar = 0.01, 100.0

    class Pipe:
        depth_ratio, compute_cov3D_python = 0.0, False

    class WithMask(Pipe):
        pass
    model = RawTrainState.from_activated(act, "cuda").model(3)
    bg = torch.zeros(3, device="cuda")
    xyz = model.get_xyz.detach()

    def same(a, b, what):
        assert a.keys() == b.keys()
        n = 0
        for k in a:
            if torch.is_tensor(a[k]):
                assert bits(a[k]) == bits(b[k]), (what, k)
                n += 1
        assert n >= 10 and float(a["render"].abs().max()) > 0

    with torch.no_grad():
        by_sphere = render(View, model, Pipe, bg, env_scope_center=list(c), env_scope_radius=r)
        WithMask.gsr_env_scope_mask = env_scope_masks(xyz, c, r)[0]
        same(render(View, model, WithMask, bg), by_sphere, "the kernel's inside mask")
        # env_scope_center / env_scope_radius are not evaluated when the pipe carries a mask
        same(render(View, model, WithMask, bg, env_scope_center=[9.0, 9.0, 9.0], env_scope_radius=0.5), by_sphere, "sphere arguments ignored")
        assert 0 < float(by_sphere["env_scope_mask"].sum()) < float(render(View, model, Pipe, bg)["env_scope_mask"].sum())
        # without the attribute the path is the parent's: its expression, restated here and handed over as the mask, renders the same bits
        centre = torch.tensor([float(v) for v in c], device="cuda")
        WithMask.gsr_env_scope_mask = ((xyz - centre[None]) ** 2).sum(dim=-1) < r ** 2
        same(render(View, model, WithMask, bg), by_sphere, "the parent's expression as the mask")
        WithMask.gsr_env_scope_mask = torch.ones(SP_, dtype=torch.bool, device="cuda")
        same(render(View, model, WithMask, bg), render(View, model, Pipe, bg), "no scope: all true")
        for bad in (torch.ones(SP_, device="cuda"), torch.ones(SP_ - 1, dtype=torch.bool, device="cuda"), torch.ones(SP_, dtype=torch.bool)):
            WithMask.gsr_env_scope_mask = bad
            with pytest.raises(ValueError):
                render(View, model, WithMask, bg)


def test_dist_color_follows_the_reference_and_zeroes_the_f_dc_moments():
    from gsr_train import RawTrainState
    sc, act, cam, ct, c, r = _scene()
    st = RawTrainState.from_activated(act, "cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    st.grads.flat.copy_(1e-3 * torch.randn(st.params.total, device="cuda", generator=g))
    st.optimizer.step()                                            # a real step: every moment is non-zero now
    st.grads.zero_()
    value, inside, outside = st.refl_scope_loss(c, r, accumulate=False)
    msk = outside | (st.a["refl_strengths"].detach() > 0.1).flatten()
    assert 0 < int(msk.sum()) < SP_
    noise = torch.rand(SP_, 1, 3, device="cuda", generator=g)
    before = {k: t.clone() for k, t in (("raw", st.params.flat), ("m", st.optimizer.exp_avg), ("v", st.optimizer.exp_avg_sq), ("act", st.optimizer.act))}
    shs0 = st.p["shs"].detach().clone()
    M = shs0.shape[1]
    # scene/gaussian_model.py:279-282 with the noise given, on the same device
    dcc = shs0[:, 0:1, :].clone()
    dist_dcc = dcc + (noise * 0.4 * 2 - 0.4)
    dist_dcc[msk] = dcc[msk]
    st.dist_color(0.4, exclusive_msk=msk, noise=noise)
    torch.cuda.synchronize()
    shs1 = st.p["shs"].detach()
    assert bits(shs1[:, 0:1, :].contiguous()) == bits(dist_dcc)
    assert bits(shs1[msk][:, 0, :].contiguous()) == bits(shs0[msk][:, 0, :].contiguous())
    assert bool((shs1[~msk][:, 0, :] != shs0[~msk][:, 0, :]).any(dim=1).all())
    assert bits(shs1[:, 1:, :].contiguous()) == bits(shs0[:, 1:, :].contiguous())
    want = E.dist_color(shs0[:, 0, :].cpu().numpy(), noise.cpu().numpy(), 0.4, msk.cpu().numpy())
    assert np.abs(shs1[:, 0, :].cpu().numpy().astype(np.float64) - want).max() <= 4 * ULP * max(1.0, np.abs(want).max())
    a, b = st.params.slices["shs"]
    assert b - a == SP_ * M * 3
    dc = torch.zeros(st.params.total, dtype=torch.bool, device="cuda")
    dc[a:b].view(SP_, M * 3)[:, :3] = True
    for q, t in (("m", st.optimizer.exp_avg), ("v", st.optimizer.exp_avg_sq)):
        assert bool((before[q][dc] != 0).all()), q                 # they were set
        assert not bool(t[dc].any()), q
        assert bits(t[~dc]) == bits(before[q][~dc]), q             # f_rest and every other group
    other = torch.ones(st.params.total, dtype=torch.bool, device="cuda")
    other[a:b] = False
    assert bits(st.params.flat[other]) == bits(before["raw"][other])
    assert bits(st.optimizer.act) == bits(before["act"])
    # noise drawn inside, [P,3] noise, no mask
    st.dist_color(0.4, exclusive_msk=msk)
    assert bits(st.p["shs"].detach()[msk][:, 0, :].contiguous()) == bits(shs0[msk][:, 0, :].contiguous())
    shs2 = st.p["shs"].detach().clone()
    st.dist_color(0.25, noise=noise.reshape(SP_, 3))
    assert bits(st.p["shs"].detach()[:, 0, :].contiguous()) == bits(shs2[:, 0, :] + (noise.reshape(SP_, 3) * 0.25 * 2 - 0.25))
