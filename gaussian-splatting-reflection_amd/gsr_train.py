"""Training-step harness around the rasterizer (reference: train.py:120-306 and
scene/gaussian_model.py:187-223): parameters, gradients and Adam moments of all eight optimizer groups live in FOUR flat
float32 buffers with one layout, so that

  * the rasterizer backward writes its gradients straight into the gradient buffer (gradient sink),
  * the multi-GPU exchange is ONE all-reduce of that buffer (gsr_dist.FlatGrads),
  * the optimizer is ONE fused Adam launch over the buffers (gsr_adam_step, include/gsr_hip.h).

The reference keeps `_features_dc` (P,1,3) and `_features_rest` (P,15,3) as separate parameters and concatenates them
for every render (scene/gaussian_model.py:135-139); here `shs` (P,16,3) is stored concatenated and the two learning
rates (feature_lr and feature_lr / 20, scene/gaussian_model.py:198-199) are applied by position inside each 48-float row.

GaussianTrainState steps whatever numbers the buffer holds (callers hand it activated values); RawTrainState holds the reference's raw
parameters and steps them through their activations in the same single launch (gsr_adam_act_step, include/gsr_hip_train.h).
"""
import ctypes
import math

import torch

import _gsr
from _gsr import AdamSegment, check, lib, stream_ptr
from gsr_dist import FlatGrads

# arguments/__init__.py:82-102 of the reference (OptimizationParams defaults)
DEFAULT_LRS = dict(position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01, position_lr_max_steps=30_000,
                   feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, refl_lr=0.006, envmap_cubemap_lr=0.05)


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/general_utils.py:29-62 of the reference: log-linear interpolation with an optional warm-up delay."""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        else:
            delay_rate = 1.0
        t = min(max(step / max_steps, 0.0), 1.0)
        log_lerp = math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
        return delay_rate * log_lerp
    return helper


class FlatParams:
    """Leaf tensors that are views of one flat float32 buffer (order of `tensors` = order in the buffer; every slice
    starts on a 16-byte boundary so the fused Adam kernel can use float4 accesses across group borders)."""

    def __init__(self, tensors, device, shapes=None, shards=1):
        """tensors: dict name -> initial value; or None with `shapes` (dict name -> shape) for an uninitialised store.
        shards > 1: the buffer length is rounded up to a multiple of 4 * shards floats so that it splits into `shards` equal,
        16-byte-aligned chunks (reduce-scatter / all-gather over ranks, gsr_dist.ShardedStep); the padding rides with the last group."""
        if tensors is not None:
            shapes = {k: tuple(v.shape) for k, v in tensors.items()}
        self.names = list(shapes.keys())
        self.shapes = {k: tuple(v) for k, v in shapes.items()}
        self.slices = {}
        off = 0
        for k in self.names:
            n = 1
            for d in self.shapes[k]:
                n *= int(d)
            self.slices[k] = (off, off + n)
            off += (n + 3) // 4 * 4
        q = 4 * max(1, int(shards))
        self.total = (off + q - 1) // q * q
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.p = {}
        for k in self.names:
            a, b = self.slices[k]
            if tensors is not None:
                self.flat[a:b].copy_(tensors[k].reshape(-1).to(device=device, dtype=torch.float32))
            self.p[k] = self.flat[a:b].view(self.shapes[k]).requires_grad_(True)

    def like(self):
        return torch.zeros_like(self.flat)

    def view_of(self, flat, name):
        a, b = self.slices[name]
        return flat[a:b].view(self.shapes[name])

    def segment(self, name):
        """(begin, end) of a group in the flat buffers with the padding that rides with it (what the fused Adam steps as that group): the
        next group's begin is its end, the last group ends at `total`."""
        i = self.names.index(name)
        return self.slices[name][0], (self.slices[self.names[i + 1]][0] if i + 1 < len(self.names) else self.total)


def copy_groups(pairs, old, new, names, segments=False):
    """dst <- src for the groups `names` in every (src, dst) pair of flat buffers laid out as `old` and `new` (FlatParams): each group's
    slice, or with `segments` its segment, padding included."""
    with torch.no_grad():
        for k in names:
            (a, b), (c, d) = (old.segment(k), new.segment(k)) if segments else (old.slices[k], new.slices[k])
            n = min(b - a, d - c)      # (the last group's padding may differ; what lies beyond the shorter one is padding on both sides)
            for src, dst in pairs:
                dst[c:c + n].copy_(src[a:a + n])


class FlatAdam:
    """torch.optim.Adam(l, lr=0.0, eps=1e-15) of scene/gaussian_model.py:196-209 over FlatParams, one kernel launch
    per step.  `groups`: name -> lr or (lr, lr2, period, split) (see gsr_adam_segment in include/gsr_hip.h)."""

    def __init__(self, params, grads_flat, groups, betas=(0.9, 0.999), eps=1e-15, owned=None):
        """owned = (begin, end) (multiples of 4): this optimizer only ever steps that range of the flat buffer (one rank's shard of a
        sharded step) and keeps Adam moments for it alone — 1/N of the moment memory."""
        self.params, self.grad = params, grads_flat
        if grads_flat.numel() != params.total or grads_flat.data_ptr() % 16 or params.flat.data_ptr() % 16:
            raise ValueError("gradient buffer must mirror the parameter buffer (same length, 16-byte aligned)")
        self.owned = (0, params.total) if owned is None else (int(owned[0]), int(owned[1]))
        a, b = self.owned
        if not (0 <= a <= b <= params.total) or a % 4 or (b % 4 and b != params.total):
            raise ValueError("owned range must lie inside the buffer with multiples of 4 as bounds")
        self.exp_avg = torch.zeros(b - a, dtype=torch.float32, device=params.flat.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.betas, self.eps, self.step_count = betas, eps, 0
        self.groups = {k: (groups[k] if isinstance(groups[k], tuple) else (float(groups[k]), 0.0, 0, 0)) for k in params.names}

    def set_lr(self, name, lr):
        g = self.groups[name]
        self.groups[name] = (float(lr),) + tuple(g[1:])

    def _table(self, struct, extra=lambda name: ()):
        """The segment table of the layout: one `struct` (begin, end, lr, lr2, period, split, *extra(name)) per group."""
        names = self.params.names
        return (struct * len(names))(*[struct(*self.params.segment(k), *self.groups[k], *extra(k)) for k in names])

    def _segments(self):
        return self._table(AdamSegment)

    def zero_moments(self, name):
        """Both moments of one group zeroed, padding included (replace_tensor_to_optimizer, scene/gaussian_model.py:395-408): the part of
        the group's segment that lies in the owned range."""
        (a, b), (lo, hi) = self.params.segment(name), self.owned
        a, b = max(a, lo) - lo, max(min(b, hi), lo) - lo
        self.exp_avg[a:b].zero_()
        self.exp_avg_sq[a:b].zero_()

    def _launch(self, buffers, rest):
        """(status, name) of the entry that takes the step: `buffers` are the pointers of param, grad, exp_avg and exp_avg_sq, `rest` every
        argument behind the segment table."""
        segs = self._segments()
        return lib.gsr_adam_step_range(*buffers, self.params.total, segs, len(segs), *rest), "gsr_adam_step"

    def step(self):
        """One Adam step over the owned range (the whole buffer unless `owned` was given)."""
        self.step_count += 1
        dev = self.params.flat.device
        _gsr.side_join(dev)      # (the cubemap gradient may still be in flight on the library's side stream)
        a, b = self.owned
        # the kernel indexes all four buffers with the GLOBAL element index; the moment buffers only exist for [a, b), so their base
        # pointers are moved back by `a` elements (a is a multiple of 4: still 16-byte aligned; nothing outside [a, b) is touched)
        buffers = (self.params.flat.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr() - 4 * a, self.exp_avg_sq.data_ptr() - 4 * a)
        with torch.cuda.device(dev):
            check(*self._launch(buffers, (self.betas[0], self.betas[1], self.eps, self.step_count, a, b, stream_ptr(dev))))


class GaussianTrainState:
    """The optimizer side of the reference's GaussianModel.training_setup (scene/gaussian_model.py:187-223) for the
    surfel + reflection model: groups xyz, f_dc / f_rest (inside shs), opacity, scaling, rotation, refl, env."""

    ORDER = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths", "cubemap", "fail")

    def __init__(self, tensors, device, spatial_lr_scale=1.0, lrs=None, _params=None, shard=None):
        """shard = (rank, world_size): this rank owns chunk `rank` of `world_size` equal chunks of the flat buffers — its optimizer steps only
        that chunk and keeps moments only for it (gsr_dist.ShardedStep moves gradients in and parameters out)."""
        lr = dict(DEFAULT_LRS)
        lr.update(lrs or {})
        self.lrs, self.spatial_lr_scale = lr, spatial_lr_scale
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        self.params = _params if _params is not None else FlatParams({k: tensors[k] for k in self.ORDER if k in tensors}, device,
                                                                     shards=1 if shard is None else self.shard[1])
        self.p = self.params.p
        self.grads = FlatGrads.mirroring(self.params)
        M = self.params.shapes["shs"][1]
        groups = dict(means3D=lr["position_lr_init"] * spatial_lr_scale,
                      shs=(lr["feature_lr"], lr["feature_lr"] / 20.0, 3 * M, 3),
                      opacities=lr["opacity_lr"], scales=lr["scaling_lr"], rotations=lr["rotation_lr"], refl_strengths=lr["refl_lr"],
                      cubemap=lr["envmap_cubemap_lr"], fail=lr["envmap_cubemap_lr"])
        owned = None
        if self.shard is not None:
            n = self.params.total // self.shard[1]
            owned = (self.shard[0] * n, (self.shard[0] + 1) * n)
        self.optimizer = self._make_optimizer({k: groups[k] for k in self.params.names}, owned)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=lr["position_lr_init"] * spatial_lr_scale,
                                                    lr_final=lr["position_lr_final"] * spatial_lr_scale,
                                                    lr_delay_mult=lr["position_lr_delay_mult"], max_steps=lr["position_lr_max_steps"])

    def _make_optimizer(self, groups, owned):
        return FlatAdam(self.params, self.grads.flat, groups, owned=owned)

    def successor(self, shapes):
        """A state of this class on a new layout (`shapes`: name -> shape, in the order of the groups; the same shard count) that goes on
        where this one stands: spatial_lr_scale, lrs, shard, optimizer.groups (the scheduled means3D rate included), step_count, betas and
        eps are carried over.  Parameters, gradient slots and moments are zero: filling them is the caller's part."""
        new = FlatParams(None, self.params.flat.device, shapes=shapes, shards=1 if self.shard is None else self.shard[1])
        st = type(self)(None, new.flat.device, spatial_lr_scale=self.spatial_lr_scale, lrs=self.lrs, _params=new, shard=self.shard)
        old, opt = self.optimizer, st.optimizer
        opt.groups, opt.step_count, opt.betas, opt.eps = dict(old.groups), old.step_count, old.betas, old.eps
        return st

    def update_learning_rate(self, iteration):
        # scene/gaussian_model.py:215-221
        v = self.xyz_scheduler_args(iteration)
        self.optimizer.set_lr("means3D", v)
        return v

    def _activated(self, name):
        """What the rasterizer reads for group `name` (RawTrainState: the activated copy)."""
        return self.p[name]

    def refl_scope_loss(self, center, radius, weight=0.4, accumulate=True):
        """The env-scope branch of the reference's iteration (train.py:56-63, 176-179) for the sink-driven step:
            loss += weight * refl[outside].mean(),   outside = sum((xyz - center)^2, -1) > radius^2
        Reads p["means3D"] and the activated reflection strengths, adds weight / count on the outside rows straight into
        grads.view("refl_strengths") — both state classes keep dL/d(activated) there, so the raw step's chain rule applies as it is —
        and returns (weight * loss detached, inside, outside): `inside` for pipe.gsr_env_scope_mask, `outside` for the exclusive masks of
        the resets.  One forward and one backward launch, no autograd node, no host read (utils.loss_utils.refl_scope_loss is the autograd
        form).  With no point outside the value is NaN, as in the reference, and the gradient buffer gets zeros or nothing.
        Ordering: call it AFTER the rasterizer's backward with accumulate=True (it adds to what the sink holds); or call it FIRST with
        accumulate=False (it overwrites the whole refl_strengths slot) and give the rasterizer's sink accumulate=True.
        A sharded state (shard=) raises NotImplementedError."""
        if self.shard is not None:
            # every rank would add the whole term to its buffer and the reduce-scatter would sum it world_size times
            raise NotImplementedError("refl_scope_loss on a sharded state (shard=(rank, world_size)) is not implemented")
        from utils import loss_utils as lu
        _gsr.require_entry(lu.lib, "gsr_env_scope_forward")
        with torch.no_grad():
            x = lu._scope_xyz(self.p["means3D"])
            refl = self._activated("refl_strengths").detach()
            inside, outside, sums = lu._scope_forward(x, refl.float().contiguous(), lu._scope_sphere(center, radius))
            g = torch.full((1,), float(weight), dtype=torch.float32, device=x.device)
            lu._scope_backward(outside, sums, g, self.grads.view("refl_strengths"), accumulate)
            return weight * (sums[0] / sums[1]), inside, outside


# ---------------------------------------------------------------------------------------------------------------------
# Raw parameters (scene/gaussian_model.py:42-52, 123-147): the reference trains _opacity, _scaling, _rotation and _refl_strength and
# renders sigmoid / exp / normalize / sigmoid of them.  Here the flat buffer holds those RAW values, a second compact buffer holds
# their activated copy for the rasterizer, and one launch (gsr_adam_act_step, include/gsr_hip_train.h) turns the dL/d(activated) the
# rasterizer wrote into dL/d(raw), steps Adam and refreshes the copy.
ACTIVATIONS = dict(opacities=_gsr.GSR_ACT_SIGMOID, scales=_gsr.GSR_ACT_EXP, rotations=_gsr.GSR_ACT_NORMALIZE4, refl_strengths=_gsr.GSR_ACT_SIGMOID)


def inverse_sigmoid(x):
    """utils/general_utils.py:18-19 of the reference."""
    return torch.log(x / (1 - x))


class RawAdam(FlatAdam):
    """FlatAdam over RAW parameters: `act` is the compact activated buffer, `act_slices[name] = (begin, end)` the place of each activated
    group in it (multiples of 4, as long as the group's segment of the flat buffer, padding included).  step() is one launch of
    gsr_adam_act_step; activate() fills `act` from the raw buffer alone (gsr_activate)."""

    def __init__(self, params, grads_flat, groups, act, act_slices, betas=(0.9, 0.999), eps=1e-15):
        _gsr.require_entry(lib, "gsr_adam_act_step")
        super().__init__(params, grads_flat, groups, betas=betas, eps=eps)
        if act.data_ptr() % 16:
            raise ValueError("the activated buffer must be 16-byte aligned")
        self.act, self.act_slices, self.frozen = act, dict(act_slices), set()

    def _act_segments(self):
        def kind_and_place(k):
            kind = ACTIVATIONS.get(k, _gsr.GSR_ACT_NONE) if k in self.act_slices else _gsr.GSR_ACT_NONE
            return kind | (_gsr.GSR_ACT_FROZEN if k in self.frozen else 0), self.act_slices[k][0] if k in self.act_slices else 0
        return self._table(_gsr.ActSegment, kind_and_place)

    def _launch(self, buffers, rest):
        segs = self._act_segments()
        return lib.gsr_adam_act_step(*buffers, self.act.data_ptr(), self.params.total, self.act.numel(), segs, len(segs), *rest), "gsr_adam_act_step"

    def activate(self):
        """act = act(raw): at construction, after densification and after a reset."""
        segs = self._act_segments()
        dev = self.params.flat.device
        with torch.cuda.device(dev):
            check(lib.gsr_activate(self.params.flat.data_ptr(), self.act.data_ptr(), self.params.total, self.act.numel(), segs, len(segs),
                                   stream_ptr(dev)), "gsr_activate")


class _Env:
    """What render() and render_env_map() take of a CubemapEncoder: `params` under the reference's keys and, called with directions [B, 3],
    the lookup of a default encoder (linear, seamless) on those two tensors, [B, C]."""

    def __init__(self, cubemap, fail):
        self.params = {"Cubemap_texture": cubemap, "Cubemap_failv": fail}

    def __call__(self, dirs):
        from cubemapencoder.cubemap_encoder import CubemapEncoder, _interp_to_id, cubemap_encode
        return cubemap_encode(dirs, self.params["Cubemap_texture"], self.params["Cubemap_failv"], _interp_to_id["linear"],
                              CubemapEncoder.seamless).permute(1, 0)


class _Model:
    """The `get_xyz / get_opacity / ...` object gaussian_renderer.render() takes (the reference's GaussianModel properties)."""

    def __init__(self, inputs, active_sh_degree):
        self.get_xyz, self.get_features = inputs["means3D"], inputs["shs"]
        self.get_opacity, self.get_scaling, self.get_rotation = inputs["opacities"], inputs["scales"], inputs["rotations"]
        self.get_refl = inputs["refl_strengths"]
        self.active_sh_degree, self.get_envmap = active_sh_degree, _Env(inputs.get("cubemap"), inputs.get("fail"))


class RawTrainState(GaussianTrainState):
    """GaussianTrainState over the reference's RAW parameters (same constructor arguments, learning rates and update_learning_rate).

      .p      leaf views of the raw flat buffer (logits, log-scales, unnormalised quaternions): what PLY export and densification read
      .a      leaf views of the compact activated buffer for opacities, scales, rotations, refl_strengths: what the rasterizer reads
      .grads  FlatGrads.mirroring(params), unchanged.  The slots of the four activated groups receive dL/d(ACTIVATED) — through the
              rasterizer's gradient sink, or through autograd (`.a[k].grad` is the view of that slot) — and optimizer.step() applies
              the chain rule itself.  (`.p[k].grad` of those four is the same view: it does not hold dL/d(raw).)
    """

    ACTIVATED = ("opacities", "scales", "rotations", "refl_strengths")

    def __init__(self, tensors, device, spatial_lr_scale=1.0, lrs=None, _params=None, shard=None):
        if shard is not None:
            raise NotImplementedError("RawTrainState(shard=...): the sharded exchange of the activated copy is not implemented; "
                                      "gsr_adam_act_step takes a range for it")
        _gsr.require_entry(lib, "gsr_adam_act_step")
        super().__init__(tensors, device, spatial_lr_scale=spatial_lr_scale, lrs=lrs, _params=_params, shard=None)
        self.a = {}
        for k, (a, b) in self.optimizer.act_slices.items():
            n = self.params.slices[k][1] - self.params.slices[k][0]
            self.a[k] = self.optimizer.act[a:a + n].view(self.params.shapes[k]).requires_grad_(True)
            self.a[k].grad = self.grads.view(k)
        self.optimizer.activate()

    def _make_optimizer(self, groups, owned):
        act_slices, off = {}, 0
        for k in self.params.names:
            if k in self.ACTIVATED:
                a, b = self.params.segment(k)
                act_slices[k] = (off, off + b - a)
                off += b - a
        act = torch.zeros(max(off, 4), dtype=torch.float32, device=self.params.flat.device)
        return RawAdam(self.params, self.grads.flat, groups, act, act_slices)

    @classmethod
    def from_activated(cls, tensors, device, **kw):
        """A state from ACTIVATED values (what gsr_init.init_from_point_cloud returns and GaussianTrainState takes): log of the scales,
        inverse_sigmoid of opacities and reflection strengths, quaternions as they are — applied once, with torch ops.  The activated copy
        starts as the very values given (exp(log(x)) is not x in float32), so that what is rendered before the first step is what
        GaussianTrainState renders from the same tensors bit for bit; the first step, a reset or a densification replaces it by act(raw)."""
        raw = dict(tensors)
        with torch.no_grad():
            for k in ("opacities", "refl_strengths"):
                if k in raw:
                    raw[k] = inverse_sigmoid(raw[k].float())
            if "scales" in raw:
                raw["scales"] = torch.log(raw["scales"].float())
        st = cls(raw, device, **kw)
        with torch.no_grad():
            for k, view in st.a.items():
                view.copy_(tensors[k].reshape(view.shape))
        return st

    def successor(self, shapes):
        st = super().successor(shapes)
        st.optimizer.frozen = set(self.optimizer.frozen)      # (the activated copy is the caller's part, as the parameters are)
        return st

    def render_inputs(self):
        """The eight tensors to hand to the rasterizer: raw means3D, shs, cubemap, fail; activated opacities, scales, rotations, refl_strengths."""
        return {k: (self.a[k] if k in self.a else self.p[k]) for k in self.params.names}

    def model(self, active_sh_degree=3):
        return _Model(self.render_inputs(), active_sh_degree)

    def _activated(self, name):
        return self.a[name] if name in self.a else self.p[name]

    def set_lr(self, name, lr):
        self.optimizer.set_lr(name, lr)

    def freeze(self, names, frozen=True):
        """freeze_xyz of the reference is freeze(("means3D", "rotations")): the step leaves those groups' raw values, moments and activated
        copy bit for bit."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [k for k in names if k not in self.params.names]
        if unknown:
            raise KeyError(f"freeze: unknown group(s) {unknown}")
        (self.optimizer.frozen.update if frozen else self.optimizer.frozen.difference_update)(names)

    def _replace(self, name, new_raw):
        """replace_tensor_to_optimizer (scene/gaussian_model.py:395-408): new raw values, both moments of the group zeroed; then the
        activated copy is refreshed."""
        with torch.no_grad():
            self.p[name].copy_(new_raw)
        self.optimizer.zero_moments(name)
        self.optimizer.activate()

    def reset_opacity(self, reset_value=0.01, exclusive_msk=None):
        # scene/gaussian_model.py:271-276
        with torch.no_grad():
            raw = self.p["opacities"].detach()
            act = torch.sigmoid(raw)
            new = inverse_sigmoid(torch.min(act, torch.ones_like(act) * reset_value))
            if exclusive_msk is not None:
                new[exclusive_msk] = raw[exclusive_msk]
        self._replace("opacities", new)

    def reset_refl(self, init_refl_value=1e-3, exclusive_msk=None):
        # scene/gaussian_model.py:264-269
        with torch.no_grad():
            raw = self.p["refl_strengths"].detach()
            act = torch.sigmoid(raw)
            new = inverse_sigmoid(torch.max(act, torch.ones_like(act) * init_refl_value))
            if exclusive_msk is not None:
                new[exclusive_msk] = raw[exclusive_msk]
        self._replace("refl_strengths", new)

    def reset_scale(self, enlarge_scale=1.5, exclusive_msk=None):
        # scene/gaussian_model.py:286-294: every axis but the smallest grows by enlarge_scale
        with torch.no_grad():
            raw = self.p["scales"].detach()
            scales = torch.exp(raw)
            min_axis_id = torch.argmin(scales, dim=-1, keepdim=True)
            rmin_axis = (torch.ones_like(scales) * enlarge_scale).scatter(1, min_axis_id, 1)
            new = torch.log(scales * rmin_axis)
            if exclusive_msk is not None:
                new[exclusive_msk] = raw[exclusive_msk]
        self._replace("scales", new)

    def dist_color(self, noise_range=0.4, exclusive_msk=None, noise=None):
        """The colour sabotage (scene/gaussian_model.py:278-284): uniform noise in [-noise_range, noise_range) on the DC colour of every
        row outside exclusive_msk, and — replace_tensor_to_optimizer on the whole f_dc group — both Adam moments zeroed at the f_dc
        positions (the first 3 floats of each 3*M-float row of shs) of ALL rows.  The f_rest moments, every other group and the activated
        copy stay bit for bit.  noise: uniform in [0, 1), [P,1,3] or [P,3] (torch.rand when None), as densify_and_prune(noise=) takes it."""
        with torch.no_grad():
            shs = self.p["shs"].detach()
            P, M = shs.shape[0], shs.shape[1]
            dcc = shs[:, 0, :].clone()
            noise = torch.rand_like(dcc) if noise is None else noise.to(device=dcc.device, dtype=torch.float32).reshape(P, 3)
            new = dcc + (noise * noise_range * 2 - noise_range)
            if exclusive_msk is not None:
                new[exclusive_msk] = dcc[exclusive_msk]
            shs[:, 0, :] = new
            a = self.params.slices["shs"][0]
            for moment in (self.optimizer.exp_avg, self.optimizer.exp_avg_sq):
                moment[a:a + P * M * 3].view(P, M * 3)[:, :3].zero_()
