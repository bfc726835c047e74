"""The raw-parameter step (include/gsr_hip_train.h: gsr_adam_act_step, gsr_activate) restated in float64 numpy, and the same chain
written with torch's own operators (torch.sigmoid / exp / nn.functional.normalize, autograd, torch.optim.Adam(lr=0, eps=1e-15)) in a
dtype of the caller's choice.  Not a test: tests/test_raw_step_ref.py pins the first against the second in float64, and the GPU tests take
the first as their yardstick and the second, in float32 on the CPU, as the measure of what float32 can deliver.

A segment is a `Seg`: the fields of gsr_act_segment.  `step()` works over flat arrays laid out as the entry's buffers are."""
import collections

import numpy as np

NONE, SIGMOID, EXP, NORMALIZE4, FROZEN = 0, 1, 2, 3, 0x100
NORM_EPS = 1e-12        # eps of torch.nn.functional.normalize
ACTIVATED = dict(opacities=SIGMOID, scales=EXP, rotations=NORMALIZE4, refl_strengths=SIGMOID)

Seg = collections.namedtuple("Seg", "begin end lr lr2 period split kind act_begin")


def segments_of(params, groups, frozen=()):
    """[Seg] and the length of the activated buffer for a gsr_train.FlatParams layout: a group's segment runs to the next group's begin
    (padding rides with the group), the activated groups get consecutive slots of their segments' lengths.  groups: name -> lr or
    (lr, lr2, period, split)."""
    segs, off = [], 0
    for i, k in enumerate(params.names):
        a = params.slices[k][0]
        end = params.slices[params.names[i + 1]][0] if i + 1 < len(params.names) else params.total
        g = groups[k] if isinstance(groups[k], tuple) else (float(groups[k]), 0.0, 0, 0)
        kind = ACTIVATED.get(k, NONE)
        # (learning rates as the float32 fields of the table carry them: every chain steps with the same numbers)
        segs.append(Seg(a, end, f32(g[0]), f32(g[1]), g[2], g[3], kind | (FROZEN if k in frozen else 0), off if kind != NONE else 0))
        if kind != NONE:
            off += end - a
    return segs, off


def element_lr(seg):
    """The learning rate of every element of a segment (gsr_adam_segment: lr for the first `split` of every `period`, lr2 for the rest)."""
    n = seg.end - seg.begin
    if seg.period == 0:
        return np.full(n, seg.lr, np.float64)
    return np.where(np.arange(n) % seg.period < seg.split, np.float64(seg.lr), np.float64(seg.lr2))


def activation(kind, r):
    """act(r) in float64; NORMALIZE4 takes whole rows of 4 (a flat array of 4k elements)."""
    kind &= 0xFF
    r = np.asarray(r, np.float64)
    if kind == SIGMOID:
        return 1.0 / (1.0 + np.exp(-r))
    if kind == EXP:
        return np.exp(r)
    if kind == NORMALIZE4:
        q = r.reshape(-1, 4)
        return (q / np.maximum(np.sqrt((q * q).sum(axis=1, keepdims=True)), NORM_EPS)).reshape(r.shape)
    return r.copy()


def raw_gradient(kind, r, g):
    """dL/d raw from dL/d activated, the activation evaluated at r."""
    kind &= 0xFF
    r, g = np.asarray(r, np.float64), np.asarray(g, np.float64)
    if kind == SIGMOID:
        # a (1 - a) with 1 - a = 1 / (1 + exp(r)) formed on its own: no cancellation at large logits
        return g * (1.0 / (1.0 + np.exp(-r))) * (1.0 / (1.0 + np.exp(r)))
    if kind == EXP:
        return g * np.exp(r)
    if kind == NORMALIZE4:
        q, gg = r.reshape(-1, 4), g.reshape(-1, 4)
        norm = np.sqrt((q * q).sum(axis=1, keepdims=True))
        safe = np.maximum(norm, NORM_EPS)
        qh = q / safe
        out = np.where(norm > NORM_EPS, (gg - qh * (qh * gg).sum(axis=1, keepdims=True)) / safe, gg / NORM_EPS)
        return out.reshape(r.shape)
    return g.copy()


def step(raw, grad, m, v, act, segs, t, betas=(0.9, 0.999), eps=1e-15, rng=None):
    """One step t (1-based) of gsr_adam_act_step over elements rng = (begin, end) (default: all) in float64.  Returns a dict of new arrays:
    raw_grad (what entered Adam; 0 where nothing did), raw, m, v, act.  Frozen segments and everything outside rng come back unchanged."""
    raw, m, v, act = (np.array(x, np.float64) for x in (raw, m, v, act))
    grad = np.asarray(grad, np.float64)
    b1, b2 = float(betas[0]), float(betas[1])
    bc1, sqrt_bc2 = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
    lo, hi = (0, raw.size) if rng is None else rng
    raw_grad = np.zeros_like(raw)
    for s in segs:
        a, b = max(s.begin, lo), min(s.end, hi)
        if a >= b or (s.kind & FROZEN):
            continue
        sl = slice(a, b)
        g = raw_gradient(s.kind, raw[sl], grad[sl])
        raw_grad[sl] = g
        m[sl] = b1 * m[sl] + (1.0 - b1) * g
        v[sl] = b2 * v[sl] + (1.0 - b2) * (g * g)
        raw[sl] -= (element_lr(s)[a - s.begin:b - s.begin] / bc1) * (m[sl] / (np.sqrt(v[sl]) / sqrt_bc2 + eps))
        if s.kind & 0xFF:
            act[s.act_begin + a - s.begin:s.act_begin + b - s.begin] = activation(s.kind, raw[sl])
    return dict(raw_grad=raw_grad, raw=raw, m=m, v=v, act=act)


def activate(raw, act, segs):
    """gsr_activate in float64: every activated segment, frozen or not."""
    act = np.array(act, np.float64)
    for s in segs:
        if s.kind & 0xFF:
            act[s.act_begin:s.act_begin + s.end - s.begin] = activation(s.kind, np.asarray(raw, np.float64)[s.begin:s.end])
    return act


def f32(x):
    """A Python float rounded to float32: the value a `float` argument or table field of the C entry carries."""
    return float(np.float32(x))


def make_case(P, scale_dims=2, L=2, M=4, seed=0, steps=3, zero_row=True):
    """Seeded inputs of the GPU tests: logits N(0, 2), log-scales N(-3, 1), quaternions N(0, 1) with one zero row, the other groups N(0, 1);
    gradients 1e-3 N(0, 1) with 10 % exact zeros.  Returns (tensors: name -> float32 array in the trainer's group order, grads: `steps`
    dicts name -> float32 array)."""
    rs = np.random.RandomState(seed)
    t = collections.OrderedDict()
    t["means3D"] = rs.randn(P, 3)
    t["shs"] = rs.randn(P, M, 3)
    t["opacities"] = 2.0 * rs.randn(P, 1)
    t["scales"] = -3.0 + rs.randn(P, scale_dims)
    t["rotations"] = rs.randn(P, 4)
    if zero_row:
        t["rotations"][P // 2] = 0.0
    t["refl_strengths"] = 2.0 * rs.randn(P, 1)
    if L:
        t["cubemap"] = rs.randn(6, 3, L, L)
        t["fail"] = rs.randn(3)
    t = collections.OrderedDict((k, x.astype(np.float32)) for k, x in t.items())
    grads = []
    for _ in range(steps):
        grads.append({k: (1e-3 * rs.randn(*x.shape) * (rs.rand(*x.shape) >= 0.1)).astype(np.float32) for k, x in t.items()})
    return t, grads


def seed_of(P, scale_dims):
    """The seed of the GPU test's case (P, scale width); tests/test_raw_step_ref.py checks each of them on the CPU."""
    return 1000 * scale_dims + P


def rotation_exempt(params, raw_grad64, grad):
    """Mask over the flat buffer: rotation elements whose float64 raw gradient is below 1e-5 of their row's incoming gradient norm.  There
    the projection g - q (q.g) cancels, and the sign that Adam's first step takes is decided by rounding."""
    out = np.zeros(params.total, bool)
    a, b = params.slices["rotations"]
    row = np.sqrt((np.asarray(grad, np.float64)[a:b].reshape(-1, 4) ** 2).sum(axis=1))
    out[a:b] = (np.abs(raw_grad64[a:b].reshape(-1, 4)) < 1e-5 * row[:, None]).reshape(-1)
    return out


class Layout:
    """names, shapes, slices, total as gsr_train.FlatParams lays groups out: every slice begins at a multiple of 4 floats."""

    def __init__(self, arrays):
        self.names = list(arrays.keys())
        self.shapes = {k: tuple(np.shape(arrays[k])) for k in self.names}
        self.slices, off = {}, 0
        for k in self.names:
            n = int(np.prod(self.shapes[k]))
            self.slices[k] = (off, off + n)
            off += (n + 3) // 4 * 4
        self.total = off


def default_groups(names, M, lrs=None):
    """name -> lr or (lr, lr2, period, split): gsr_train.DEFAULT_LRS as GaussianTrainState assigns them (position_lr_init at scale 1)."""
    lr = dict(position_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, refl_lr=0.006, envmap_cubemap_lr=0.05)
    lr.update(lrs or {})
    g = dict(means3D=lr["position_lr_init"], shs=(lr["feature_lr"], lr["feature_lr"] / 20.0, 3 * M, 3), opacities=lr["opacity_lr"],
             scales=lr["scaling_lr"], rotations=lr["rotation_lr"], refl_strengths=lr["refl_lr"], cubemap=lr["envmap_cubemap_lr"],
             fail=lr["envmap_cubemap_lr"])
    return {k: g[k] for k in names}


def flat_from(params, arrays, dtype=np.float32):
    """Group arrays packed into one flat array of a FlatParams layout (zeros in the padding)."""
    out = np.zeros(params.total, dtype)
    for k in params.names:
        a, b = params.slices[k]
        out[a:b] = np.asarray(arrays[k]).reshape(-1)
    return out


def torch_chain(params, grads, segs, steps, dtype, betas=(0.9, 0.999), eps=1e-15):
    """The same steps with torch's own operators in `dtype` on the CPU: one leaf per group (two for a group with two learning rates, as the
    reference keeps f_dc and f_rest apart), activation -> backward(dL/d activated) -> torch.optim.Adam with per-group lr.
    params = (names, slices, shapes, raw0): a FlatParams layout and the flat array of raw values; grads: one flat array per step; segs: one
    Seg per name.  Only the elements inside each group's slice take part (torch knows no padding).  Returns per step a dict of flat float64
    arrays raw_grad, raw, m, v (zeros in the padding) and act, a list of (name, flat array) for the activated groups in layout order."""
    import torch
    names, slices, shapes, raw0 = params
    seg_of = dict(zip(names, segs))
    leaves, opt_groups = {}, []
    for k in names:
        a, b = slices[k]
        s = seg_of[k]
        x = torch.tensor(np.asarray(raw0[a:b], np.float64), dtype=dtype)
        if s.period:
            rows = x.view(-1, s.period)
            parts = [rows[:, :s.split].clone(), rows[:, s.split:].clone()]
            lrs = [s.lr, s.lr2]
        else:
            parts, lrs = [x.view(shapes[k]).clone()], [s.lr]
        for p in parts:
            p.requires_grad_(not (s.kind & FROZEN))
        leaves[k] = parts
        if not (s.kind & FROZEN):
            opt_groups += [{"params": [p], "lr": float(lr)} for p, lr in zip(parts, lrs)]
    opt = torch.optim.Adam(opt_groups, lr=0.0, eps=eps, betas=(float(betas[0]), float(betas[1])))

    def act_of(k):
        s = seg_of[k]
        kind = s.kind & 0xFF
        x = leaves[k][0]
        if kind == SIGMOID:
            return torch.sigmoid(x)
        if kind == EXP:
            return torch.exp(x)
        if kind == NORMALIZE4:
            return torch.nn.functional.normalize(x.view(-1, 4)).view(x.shape)
        return None

    def flat_of(k, fn):
        s = seg_of[k]
        parts = [fn(p) for p in leaves[k]]
        if s.period:
            return torch.cat([parts[0], parts[1]], dim=1).reshape(-1)
        return parts[0].reshape(-1)

    out = []
    total = len(raw0)
    for t in range(steps):
        opt.zero_grad(set_to_none=True)
        for k in names:
            a, b = slices[k]
            s = seg_of[k]
            if s.kind & FROZEN:
                continue
            g = torch.tensor(np.asarray(grads[t][a:b], np.float64), dtype=dtype)
            if s.period:
                rows = g.view(-1, s.period)
                leaves[k][0].grad = rows[:, :s.split].clone()
                leaves[k][1].grad = rows[:, s.split:].clone()
            elif (s.kind & 0xFF) == NONE:
                leaves[k][0].grad = g.view(shapes[k]).clone()
            else:
                act_of(k).backward(g.view(shapes[k]))
        res = {q: np.zeros(total, np.float64) for q in ("raw_grad", "raw", "m", "v")}
        for k in names:
            a, b = slices[k]
            if not (seg_of[k].kind & FROZEN):
                res["raw_grad"][a:b] = flat_of(k, lambda p: p.grad.detach().clone()).double().numpy()
        opt.step()
        res["act"] = []
        for k in names:
            a, b = slices[k]
            res["raw"][a:b] = flat_of(k, lambda p: p.detach()).double().numpy()
            if not (seg_of[k].kind & FROZEN):
                res["m"][a:b] = flat_of(k, lambda p: opt.state[p]["exp_avg"]).double().numpy()
                res["v"][a:b] = flat_of(k, lambda p: opt.state[p]["exp_avg_sq"]).double().numpy()
            if seg_of[k].kind & 0xFF:
                with torch.no_grad():
                    res["act"].append((k, act_of(k).reshape(-1).double().numpy()))
        out.append(res)
    return out
