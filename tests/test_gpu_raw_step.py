"""gsr_adam_act_step and gsr_activate (include/gsr_hip_train.h) on the GPU against tests/raw_step_ref.py, the float64 restatement that
tests/test_raw_step_ref.py pins to torch's operators.

Layouts come from gsr_train.FlatParams: P in {1, 3, 257, 1031} (slices carry padding; more than one block), scale width 2 and 3, a cubemap
group (L = 2) and the fail value behind the per-Gaussian groups; one direct call with a single SIGMOID segment of 4099 floats reaches the
scalar tail.  Inputs: raw_step_ref.make_case (logits N(0, 2), log-scales N(-3, 1), quaternions N(0, 1) with one zero row, gradients
1e-3 N(0, 1) with 10 % exact zeros).  Every chain steps with the same float32 constants (the learning rates of the table, beta1, beta2).

Tolerance, computed at run time per group and quantity: 4 x the largest error of torch's own float32 chain on the CPU (same inputs, same
steps) against the float64 restatement, plus 2 ulp (2^-23 relative) of the largest value compared.  4 x: the device's exp, division and
rsqrt may differ from libm's by an ulp or two, and Adam passes a relative gradient error one to one into the update.  The zero quaternion
row (raw gradient g / 1e-12, nine orders above its neighbours) is bounded on its own, so that it does not set the rotation group's scale.
In the rotation group an element whose float64 raw gradient is below 1e-5 of its row's incoming gradient norm is left out (with its row's
activated copy) from that step on: the projection cancels there and the sign Adam's first step takes is decided by rounding; at most 2 per
step, and tests/test_raw_step_ref.py checks on the CPU that the seeds keep the restatement within that cap."""
import functools

import numpy as np
import pytest
import torch

import raw_step_ref as R
from poison import u32

pytestmark = pytest.mark.gpu

B1, B2 = R.f32(0.9), R.f32(0.999)
ULP = 2.0 ** -23
CASES = [(P, S) for P in (1, 3, 257, 1031) for S in (2, 3)]


def _c_segments(segs):
    import _gsr
    arr = (_gsr.ActSegment * len(segs))()
    for i, s in enumerate(segs):
        arr[i] = _gsr.ActSegment(*s)
    return arr


def _step(buf, segs, t, rng=None, n_act=None):
    """gsr_adam_act_step on the device buffers buf = dict(raw, grad, m, v, act) on the current stream."""
    import _gsr
    n = buf["raw"].numel()
    lo, hi = (0, n) if rng is None else rng
    _gsr.check(_gsr.lib.gsr_adam_act_step(buf["raw"].data_ptr(), buf["grad"].data_ptr(), buf["m"].data_ptr(), buf["v"].data_ptr(), buf["act"].data_ptr(), n,
                                          buf["act"].numel() if n_act is None else n_act, _c_segments(segs), len(segs), B1, B2, 1e-15, t, lo, hi,
                                          _gsr.stream_ptr(buf["raw"].device)), "gsr_adam_act_step")


def _activate(raw, act, segs):
    import _gsr
    _gsr.check(_gsr.lib.gsr_activate(raw.data_ptr(), act.data_ptr(), raw.numel(), act.numel(), _c_segments(segs), len(segs), _gsr.stream_ptr(raw.device)),
               "gsr_activate")


def _subsets(lay, segs, exempt):
    """[(label, flat indices, act indices or None)]: one per group, the zero quaternion row apart from the other rows, exempt elements (and the
    activated copy of their rows) left out."""
    out = []
    for name, s in zip(lay.names, segs):
        a, b = lay.slices[name]
        idx = np.arange(a, b)
        aidx = s.act_begin + (idx - a) if (s.kind & 0xFF) else None
        if name == "rotations":
            ok_row = ~exempt[a:b].reshape(-1, 4).any(axis=1)
            zero = np.zeros(b - a, bool)
            P = (b - a) // 4
            zero[4 * (P // 2):4 * (P // 2) + 4] = True
            keep, keep_act = ~exempt[a:b], np.repeat(ok_row, 4)
            for label, sel in (("rotations", ~zero), ("rotations[zero row]", zero)):
                if sel.any():
                    out.append((label, idx[sel & keep], aidx[sel & keep_act]))
        else:
            out.append((name, idx, aidx))
    return out


def _bound(c32, ref, idx):
    if idx.size == 0:
        return 0.0, 0.0
    err32 = float(np.abs(c32[idx] - ref[idx]).max())
    return 4.0 * err32 + 2.0 * ULP * float(np.abs(ref[idx]).max()), err32


@functools.lru_cache(maxsize=None)
def _case(P, S, lr0=False, frozen=()):
    """Inputs, layout, segments, and both CPU chains over three steps (computed once per case, shared, never modified)."""
    t, grads = R.make_case(P, scale_dims=S, L=2, M=4, seed=R.seed_of(P, S), steps=3)
    lay = R.Layout(t)
    groups = R.default_groups(lay.names, 4)
    if lr0:
        groups = {k: ((0.0, 0.0) + g[2:] if isinstance(g, tuple) else 0.0) for k, g in groups.items()}
    segs, n_act = R.segments_of(lay, groups, frozen=frozen)
    raw0 = R.flat_from(lay, t)
    gflat = [R.flat_from(lay, g) for g in grads]
    ref, cur = [], dict(raw=raw0.astype(np.float64), m=np.zeros(lay.total), v=np.zeros(lay.total), act=R.activate(raw0, np.zeros(n_act), segs))
    exempt, newly = np.zeros(lay.total, bool), []
    for step in range(1, 4):
        cur = R.step(cur["raw"], gflat[step - 1], cur["m"], cur["v"], cur["act"], segs, step, betas=(B1, B2))
        new = R.rotation_exempt(lay, cur["raw_grad"], gflat[step - 1]) & ~exempt
        if "rotations" in frozen:
            new[:] = False
        newly.append(int(new.sum()))
        exempt = exempt | new
        ref.append(dict(cur, exempt=exempt.copy()))
    chain = R.torch_chain((lay.names, lay.slices, lay.shapes, raw0), gflat, segs, 3, torch.float32, betas=(B1, B2))
    for c in chain:                                                      # the float32 chain's activated copy in the compact layout
        act = np.zeros(n_act)
        for (name, x), s in zip(c["act"], [s for s in segs if s.kind & 0xFF]):
            act[s.act_begin:s.act_begin + x.size] = x
        c["act_flat"] = act
    return dict(t=t, lay=lay, segs=segs, n_act=n_act, raw0=raw0, grads=gflat, ref=ref, chain=chain, newly=newly)


def _device(c):
    from gsr_train import FlatParams
    fp = FlatParams({k: torch.from_numpy(v) for k, v in c["t"].items()}, "cuda")
    assert fp.slices == c["lay"].slices and fp.total == c["lay"].total and fp.names == c["lay"].names
    assert u32(fp.flat.cpu().numpy()).tobytes() == u32(c["raw0"]).tobytes()
    return dict(raw=fp.flat.detach().clone(), grad=torch.zeros(fp.total, device="cuda"), m=torch.zeros(fp.total, device="cuda"),
                v=torch.zeros(fp.total, device="cuda"), act=torch.full((c["n_act"],), float("nan"), device="cuda"))


def _compare(c, buf, step, what=("raw", "m", "v", "act"), report=None):
    ref, c32 = c["ref"][step - 1], c["chain"][step - 1]
    got = {k: buf[k].cpu().numpy().astype(np.float64) for k in ("raw", "m", "v", "act")}
    for label, idx, aidx in _subsets(c["lay"], c["segs"], ref["exempt"]):
        for q in what:
            if q == "act":
                if aidx is None:
                    continue
                bound, e32 = _bound(c32["act_flat"], ref["act"], aidx)
                err = float(np.abs(got["act"][aidx] - ref["act"][aidx]).max()) if aidx.size else 0.0
            else:
                bound, e32 = _bound(c32[q], ref[q], idx)
                err = float(np.abs(got[q][idx] - ref[q][idx]).max()) if idx.size else 0.0
            print(f"step {step} {label:22s} {q:4s} device {err:.3e}  float32 chain {e32:.3e}  bound {bound:.3e}")
            if report is not None:
                report.append((step, label, q, err, e32, bound))
            assert err <= bound, (step, label, q, err, bound)


@pytest.mark.parametrize("P,S", CASES)
def test_chain_rule_alone_with_every_learning_rate_zero(P, S):
    """One step with lr = 0 everywhere: raw stays bit for bit, exp_avg / (1 - beta1) is the float64 raw gradient within the bound (relative to
    the group's largest), the activated copy is the float64 activation of raw."""
    c = _case(P, S, lr0=True)
    buf = _device(c)
    buf["grad"].copy_(torch.from_numpy(c["grads"][0]))
    _step(buf, c["segs"], 1)
    torch.cuda.synchronize()
    assert u32(buf["raw"].cpu().numpy()).tobytes() == u32(c["raw0"]).tobytes()
    ref, c32 = c["ref"][0], c["chain"][0]
    got = buf["m"].cpu().numpy().astype(np.float64) / (1.0 - B1)
    assert c["newly"][0] <= 2
    for label, idx, aidx in _subsets(c["lay"], c["segs"], ref["exempt"]):
        bound, e32 = _bound(c32["raw_grad"], ref["raw_grad"], idx)
        err = float(np.abs(got[idx] - ref["raw_grad"][idx]).max()) if idx.size else 0.0
        scale = float(np.abs(ref["raw_grad"][idx]).max()) if idx.size else 0.0
        print(f"{label:22s} raw gradient: device {err:.3e} float32 chain {e32:.3e} bound {bound:.3e} (largest {scale:.3e})")
        assert err <= bound, (label, err, bound)
    _compare(c, buf, 1, what=("act",))


@pytest.mark.parametrize("P,S", CASES)
def test_three_steps_with_the_default_learning_rates(P, S):
    """raw, both moments and the activated copy after each of three steps; beside it gsr_adam_step on copies of the same buffers, to which the
    NONE segments are bit-identical; the activated buffer starts as NaN and holds none inside its slices afterwards; grad is not written."""
    import _gsr
    c = _case(P, S)
    buf = _device(c)
    twin = {k: buf[k].clone() for k in ("raw", "m", "v")}
    lay, segs = c["lay"], c["segs"]
    plain = (_gsr.AdamSegment * len(segs))(*[_gsr.AdamSegment(*s[:6]) for s in segs])
    assert all(n <= 2 for n in c["newly"]), c["newly"]
    for step in range(1, 4):
        buf["grad"].copy_(torch.from_numpy(c["grads"][step - 1]))
        g_bits = u32(buf["grad"].cpu().numpy()).tobytes()
        _step(buf, segs, step)
        _gsr.check(_gsr.lib.gsr_adam_step(twin["raw"].data_ptr(), buf["grad"].data_ptr(), twin["m"].data_ptr(), twin["v"].data_ptr(), lay.total, plain,
                                          len(segs), B1, B2, 1e-15, step, _gsr.stream_ptr(buf["raw"].device)), "gsr_adam_step")
        torch.cuda.synchronize()
        assert u32(buf["grad"].cpu().numpy()).tobytes() == g_bits
        act = buf["act"].cpu().numpy()
        for name, s in zip(lay.names, segs):
            a = lay.slices[name][0]
            if s.kind & 0xFF:
                assert not np.isnan(act[s.act_begin:s.act_begin + (s.end - a)]).any(), name        # the whole slot, padding included
            else:
                for q in ("raw", "m", "v"):
                    assert u32(buf[q][a:s.end].cpu().numpy()).tobytes() == u32(twin[q][a:s.end].cpu().numpy()).tobytes(), (name, q, step)
        _compare(c, buf, step)


@pytest.mark.parametrize("P,S", [(257, 2), (1031, 3)])
def test_frozen_groups_and_ranges_stay_bit_for_bit(P, S):
    """freeze_xyz (means3D and rotations frozen): raw, both moments and the activated copy of those groups keep their bits.  A step over
    [range_begin, range_end) leaves everything outside alone, and two half ranges reproduce the full step bit for bit."""
    c = _case(P, S, frozen=("means3D", "rotations"))
    lay, segs = c["lay"], c["segs"]
    buf = _device(c)
    _activate(buf["raw"], buf["act"], segs)                       # (fills the frozen groups' copy too)
    rs = np.random.RandomState(P)                                 # moments as a run in progress has them
    buf["m"].copy_(torch.from_numpy((1e-3 * rs.randn(lay.total)).astype(np.float32)))
    buf["v"].copy_(torch.from_numpy((1e-6 * rs.rand(lay.total)).astype(np.float32)))
    buf["grad"].copy_(torch.from_numpy(c["grads"][0]))
    start = {k: buf[k].clone() for k in buf}

    def bits(t):
        return u32(t.cpu().numpy())

    _step(buf, segs, 2)
    torch.cuda.synchronize()
    for name, s in zip(lay.names, segs):
        a = lay.slices[name][0]
        same = [bool((bits(buf[q][a:s.end]) == bits(start[q][a:s.end])).all()) for q in ("raw", "m", "v")]
        if s.kind & 0xFF:
            same.append(bool((bits(buf["act"][s.act_begin:s.act_begin + s.end - a]) == bits(start["act"][s.act_begin:s.act_begin + s.end - a])).all()))
        if s.kind & R.FROZEN:
            assert all(same), (name, same)
        else:
            assert not same[0] and not same[1], name
    ref = R.step(start["raw"].cpu().numpy(), c["grads"][0], start["m"].cpu().numpy(), start["v"].cpu().numpy(), start["act"].cpu().numpy(), segs, 2,
                 betas=(B1, B2))
    assert np.abs(buf["raw"].cpu().numpy() - ref["raw"]).max() <= 2e-3 * 0.05          # (a coarse check that the step is the step: lr = 0.05 at most)
    # ranges: bounds that fall inside groups, multiples of 4
    n = lay.total
    half = (n // 2) // 4 * 4
    lo, hi = (n // 5) // 4 * 4, (4 * n // 5) // 4 * 4
    part = {k: start[k].clone() for k in start}
    _step(part, segs, 2, rng=(lo, hi))
    torch.cuda.synchronize()
    for q in ("raw", "m", "v"):
        assert (bits(part[q][:lo]) == bits(start[q][:lo])).all() and (bits(part[q][hi:]) == bits(start[q][hi:])).all(), q
        assert (bits(part[q][lo:hi]) == bits(buf[q][lo:hi])).all(), q
    for name, s in zip(lay.names, segs):
        if s.kind & 0xFF:
            inside = np.zeros(s.end - s.begin, bool)
            inside[max(lo, s.begin) - s.begin:max(min(hi, s.end) - s.begin, 0)] = True
            if s.kind & R.FROZEN:
                inside[:] = False
            got, was, full = (bits(x[s.act_begin:s.act_begin + s.end - s.begin]) for x in (part["act"], start["act"], buf["act"]))
            assert (got[~inside] == was[~inside]).all() and (got[inside] == full[inside]).all(), name
    two = {k: start[k].clone() for k in start}
    _step(two, segs, 2, rng=(0, half))
    _step(two, segs, 2, rng=(half, n))
    torch.cuda.synchronize()
    for q in ("raw", "m", "v", "act"):
        assert (bits(two[q]) == bits(buf[q])).all(), q
    assert (bits(two["grad"]) == bits(start["grad"])).all()


def test_non_default_stream_and_activate_alone():
    """The same step issued on a non-default stream gives the same bits; gsr_activate alone fills the activated copy (frozen groups included)
    from raw within the bound, writes nothing else, and an empty range or n = 0 is a no-op."""
    import _gsr
    c = _case(257, 3)
    segs = c["segs"]
    a, b = _device(c), _device(c)
    for buf in (a, b):
        buf["grad"].copy_(torch.from_numpy(c["grads"][0]))
    _step(a, segs, 1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())          # (the buffers were filled on the default stream)
    with torch.cuda.stream(side):
        _step(b, segs, 1)
    side.synchronize()
    for q in ("raw", "m", "v", "act"):
        assert u32(a[q].cpu().numpy()).tobytes() == u32(b[q].cpu().numpy()).tobytes(), q
    # gsr_activate alone, with two groups frozen (the flag is ignored there), on the side stream
    cf = _case(257, 3, frozen=("means3D", "rotations"))
    d = _device(cf)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _activate(d["raw"], d["act"], cf["segs"])
    side.synchronize()
    assert u32(d["raw"].cpu().numpy()).tobytes() == u32(cf["raw0"]).tobytes()
    want = R.activate(cf["raw0"], np.zeros(cf["n_act"]), cf["segs"])
    got = d["act"].cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any()
    for name, s in zip(cf["lay"].names, cf["segs"]):
        kind = s.kind & 0xFF
        if not kind:
            continue
        lo, hi = cf["lay"].slices[name]
        x = torch.from_numpy(cf["raw0"][lo:hi])
        t32 = {R.SIGMOID: torch.sigmoid, R.EXP: torch.exp, R.NORMALIZE4: lambda q: torch.nn.functional.normalize(q.view(-1, 4)).reshape(-1)}[kind](x)
        ref = want[s.act_begin:s.act_begin + hi - lo]
        e32 = float(np.abs(t32.double().numpy() - ref).max())
        err = float(np.abs(got[s.act_begin:s.act_begin + hi - lo] - ref).max())
        print(f"gsr_activate {name:16s} device {err:.3e} float32 torch {e32:.3e}")
        assert err <= 4 * e32 + 2 * ULP * float(np.abs(ref).max()), name
    # no-ops
    before = {k: u32(a[k].cpu().numpy()).tobytes() for k in a}
    _step(a, segs, 2, rng=(8, 8))
    assert _gsr.lib.gsr_adam_act_step(None, None, None, None, None, 0, 0, None, 0, B1, B2, 1e-15, 1, 0, 0, None) == 0
    assert _gsr.lib.gsr_activate(None, None, 0, 0, None, 0, None) == 0
    torch.cuda.synchronize()
    assert before == {k: u32(a[k].cpu().numpy()).tobytes() for k in a}


def test_both_entries_agree_on_odd_borders_and_the_tail():
    """gsr_adam_step_range beside gsr_adam_act_step with the same table as GSR_ACT_NONE and act = NULL, where the layouts above never put
    them: n = 4099 (a tail of 3) and three segments with odd borders, so that float4s straddle them; the middle one has two rates by
    position.  Three steps: parameters and both moments bit-identical over all n floats, the float behind each buffer untouched."""
    import _gsr
    n = 4099
    table = [(0, 1001, 0.05, 0.0, 0, 0), (1001, 2050, 0.0025, 0.000125, 7, 3), (2050, n, 0.001, 0.0, 0, 0)]
    plain = (_gsr.AdamSegment * 3)(*[_gsr.AdamSegment(*s) for s in table])
    none = (_gsr.ActSegment * 3)(*[_gsr.ActSegment(*s, _gsr.GSR_ACT_NONE, 0) for s in table])
    rs = np.random.RandomState(4100)
    raw0 = torch.from_numpy(rs.randn(n).astype(np.float32))
    guard = 1.25
    stores = [{k: torch.full((n + 1,), guard, device="cuda") for k in ("raw", "grad", "m", "v")} for _ in range(2)]
    for store in stores:
        store["raw"][:n].copy_(raw0)
        store["m"][:n].zero_()
        store["v"][:n].zero_()
    a, b = stores
    stream = _gsr.stream_ptr(a["raw"].device)
    for step in range(1, 4):
        g = torch.from_numpy((1e-3 * rs.randn(n) * (rs.rand(n) >= 0.1)).astype(np.float32))
        for store in stores:
            store["grad"][:n].copy_(g)
        _gsr.check(_gsr.lib.gsr_adam_step_range(a["raw"].data_ptr(), a["grad"].data_ptr(), a["m"].data_ptr(), a["v"].data_ptr(), n, plain, 3, B1, B2,
                                                1e-15, step, 0, n, stream), "gsr_adam_step_range")
        _gsr.check(_gsr.lib.gsr_adam_act_step(b["raw"].data_ptr(), b["grad"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), None, n, 0, none, 3, B1, B2,
                                              1e-15, step, 0, n, stream), "gsr_adam_act_step")
        torch.cuda.synchronize()
        for q in ("raw", "m", "v"):
            assert u32(a[q][:n].cpu().numpy()).tobytes() == u32(b[q][:n].cpu().numpy()).tobytes(), (q, step)
        assert not torch.equal(a["raw"][:n].cpu(), raw0)
        assert all(float(x[n]) == guard for store in stores for x in store.values())


def test_one_sigmoid_segment_of_4099_floats_reaches_the_scalar_tail():
    """A direct call: n = 4099 = 4 * 1024 + 3, one SIGMOID segment; the last three elements take the one-element path.  Three steps against the
    restatement, bounds as above; the activated buffer is exactly n floats long and the float behind `raw`'s last is not touched."""
    n = 4099
    rs = np.random.RandomState(4099)
    raw0 = (2.0 * rs.randn(n)).astype(np.float32)
    grads = [(1e-3 * rs.randn(n) * (rs.rand(n) >= 0.1)).astype(np.float32) for _ in range(3)]
    segs = [R.Seg(0, n, R.f32(0.05), 0.0, 0, 0, R.SIGMOID, 0)]
    lay = R.Layout({"x": raw0})
    assert lay.slices["x"] == (0, n)
    chain = R.torch_chain((["x"], {"x": (0, n)}, {"x": (n,)}, raw0), grads, segs, 3, torch.float32, betas=(B1, B2))
    guard = 1.25
    store = {k: torch.full((n + 1,), guard, device="cuda") for k in ("raw", "grad", "m", "v", "act")}
    buf = {k: x[:n] for k, x in store.items()}
    buf["raw"].copy_(torch.from_numpy(raw0))
    buf["m"].zero_(); buf["v"].zero_()
    buf["act"].fill_(float("nan"))
    cur = dict(raw=raw0.astype(np.float64), m=np.zeros(n), v=np.zeros(n), act=np.zeros(n))
    idx = np.arange(n)
    for step in range(1, 4):
        buf["grad"].copy_(torch.from_numpy(grads[step - 1]))
        _step(buf, segs, step)
        torch.cuda.synchronize()
        cur = R.step(cur["raw"], grads[step - 1], cur["m"], cur["v"], cur["act"], segs, step, betas=(B1, B2))
        c32 = dict(chain[step - 1], act=chain[step - 1]["act"][0][1])
        for q in ("raw", "m", "v", "act"):
            bound, e32 = _bound(c32[q], cur[q], idx)
            got = buf[q].cpu().numpy().astype(np.float64)
            err = float(np.abs(got - cur[q]).max())
            tail = float(np.abs(got[-3:] - cur[q][-3:]).max())
            print(f"step {step} {q:4s} device {err:.3e} (tail {tail:.3e}) float32 chain {e32:.3e} bound {bound:.3e}")
            assert err <= bound, (step, q, err, bound)
        assert all(float(x[n]) == guard for x in store.values())
