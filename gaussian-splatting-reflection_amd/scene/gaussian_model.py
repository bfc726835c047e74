"""GaussianModel: the class the reference's train.py, render.py, eval_fps.py, view.py and scene/__init__.py hold (reference:
scene/gaussian_model.py), as a facade over the flat training state.

The reference keeps seven nn.Parameters, a CubemapEncoder and a torch.optim.Adam over eight groups and rebuilds all of them for every
prune / clone / split.  Here the model holds ONE gsr_train.RawTrainState (raw parameters, gradients and both Adam moments in four flat
buffers, the activated copy in a fifth) and ONE gsr_densify.DensifyStats, and every method of the reference's interface is a call into
what the library already has: the getters are views of those buffers, optimizer.step() is the one fused launch, densify_and_prune /
prune_points / double_env_map return a successor state which the model adopts.  The class adds no arithmetic of its own.

What differs from the reference, by design:
  * the activated getters (get_opacity, get_scaling, get_rotation, get_refl) are LEAVES: the activated copy the fused step keeps fresh, whose
    `.grad` is the optimizer's gradient slot.  loss.backward() therefore lands dL/d(activated) in the flat gradient buffer and
    optimizer.step() applies the chain rule through sigmoid / exp / normalize itself (gsr_adam_act_step);
  * get_features is the stored `shs` group, [P, M, 3]; _features_dc / _features_rest are views of it, not parameters of their own;
  * the model holds its flat state from create_from_pcd / load_ply / restore on (a model that is only rendered carries empty gradient and
    moment buffers along); `optimizer` is None until training_setup, as in the reference;
  * everything that is not in the reference is keyword-only: create_from_pcd(generator=), add_densification_stats(radii=),
    densify_and_prune(noise=, plan=), dist_color(noise=), bind(pipe).
A sharded model is out of scope: RawTrainState(shard=...) raises, and so does training_setup(group=...).
"""
import torch

import gsr_densify
import gsr_envmap
from _gsr import check, lib, ptr, require_entry, side_join, stream_ptr
from gsr_train import DEFAULT_LRS, RawTrainState, _Env, copy_groups

# the reference's optimizer groups (scene/gaussian_model.py:196-205), in its order, and the state's group each one lives in
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "refl", "env")
_GROUP_OF = dict(xyz="means3D", opacity="opacities", scaling="scales", rotation="rotations", refl="refl_strengths")
_PER_GAUSSIAN = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")
_ADAM_DEFAULTS = dict(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)


def _env_order():
    """The env group's two parameters as state groups, in the order list(CubemapEncoder.parameters()) gives them."""
    from cubemapencoder import CubemapEncoder
    names = [n for n, _ in CubemapEncoder(output_dim=1, resolution=1).named_parameters()]
    return [dict(Cubemap_texture="cubemap", Cubemap_failv="fail")[n.split(".")[-1]] for n in names]


class _Optimizer:
    """What the reference's loop and checkpoints use of torch.optim.Adam, over state.optimizer (gsr_train.RawAdam): step(), zero_grad(),
    param_groups, state_dict(), load_state_dict().  A caller's write to param_groups[i]["lr"] reaches the fused step with the next step()."""

    def __init__(self, model):
        self._model = model
        self._env = _env_order()
        self.param_groups = []
        self.rebind()

    @property
    def _state(self):
        return self._model._state

    def _lrs(self):
        """{reference group name: lr} as the state's segment table holds them."""
        g = self._state.optimizer.groups
        out = {n: g[k][0] for n, k in _GROUP_OF.items()}
        out.update(f_dc=g["shs"][0], f_rest=g["shs"][1], env=g["cubemap"][0])
        return out

    def rebind(self):
        """param_groups of the model's CURRENT state (after training_setup and after every successor state): `params` become that state's
        raw tensors.  The eight dicts stay the same objects, as torch.optim.Adam's do when the reference swaps a parameter: a caller that
        holds one keeps writing learning rates the next step() honours (a successor state carries them as they were pushed)."""
        m = self._model
        tensors = dict(xyz=[m._xyz], f_dc=[m._features_dc], f_rest=[m._features_rest], opacity=[m._opacity], scaling=[m._scaling],
                       rotation=[m._rotation], refl=[m._refl_strength], env=[self._state.p[k] for k in self._env])
        if not self.param_groups:
            opt, lrs = self._state.optimizer, self._lrs()
            self.param_groups = [dict(params=tensors[n], lr=lrs[n], name=n, betas=tuple(opt.betas), eps=opt.eps, **_ADAM_DEFAULTS) for n in GROUPS]
        for g in self.param_groups:
            g["params"] = tensors[g["name"]]

    def push(self):
        """The learning rates, betas and eps of param_groups into the state's segment table (the fused step reads only that)."""
        opt = self._state.optimizer
        lr = {g["name"]: float(g["lr"]) for g in self.param_groups}
        for n, k in _GROUP_OF.items():
            opt.set_lr(k, lr[n])
        shs = opt.groups["shs"]
        opt.groups["shs"] = (lr["f_dc"], lr["f_rest"]) + tuple(shs[2:])
        opt.set_lr("cubemap", lr["env"])
        opt.set_lr("fail", lr["env"])
        opt.betas, opt.eps = tuple(self.param_groups[0]["betas"]), self.param_groups[0]["eps"]

    def step(self):
        self.push()
        self._state.optimizer.step()

    def zero_grad(self, set_to_none=True):
        """Zeroes the flat gradient buffer.  Every `.grad` stays the view of its slot whatever `set_to_none` says: autograd and the gradient
        sinks accumulate into those views, and the fused step reads the buffer."""
        self._state.grads.zero_()

    # ---------------------------------------------------------------------------------------------- checkpoints
    def _slots(self):
        """[(state group, column slice inside a row of the group or None, shape)] of the nine parameters in state_dict order."""
        p = self._state.p
        P, M = p["shs"].shape[0], p["shs"].shape[1]
        out = [("means3D", None, p["means3D"].shape), ("shs", (0, 3), (P, 1, 3)), ("shs", (3, 3 * M), (P, M - 1, 3))]
        out += [(k, None, p[k].shape) for k in ("opacities", "scales", "rotations", "refl_strengths")]
        return out + [(k, None, p[k].shape) for k in self._env]

    def _moment_view(self, moment, group, cols):
        params = self._state.params
        a, b = params.slices[group]
        v = moment[a:b]
        if cols is None:
            return v.view(params.shapes[group])
        P, M = params.shapes["shs"][0], params.shapes["shs"][1]
        return v.view(P, 3 * M)[:, cols[0]:cols[1]]

    def state_dict(self):
        """The layout of torch.optim.Adam.state_dict(): "state" {0..8: step, exp_avg, exp_avg_sq} in the order xyz, f_dc, f_rest, opacity,
        scaling, rotation, refl and the env group's two parameters; "param_groups" with the indices in `params`.  Copies, not views."""
        self.push()
        opt = self._state.optimizer
        state = {}
        for i, (group, cols, shape) in enumerate(self._slots()):
            state[i] = dict(step=torch.tensor(float(opt.step_count)),
                            exp_avg=self._moment_view(opt.exp_avg, group, cols).clone(memory_format=torch.contiguous_format).reshape(shape),
                            exp_avg_sq=self._moment_view(opt.exp_avg_sq, group, cols).clone(memory_format=torch.contiguous_format).reshape(shape))
        groups, i = [], 0
        for g in self.param_groups:
            n = len(g["params"])
            groups.append(dict({k: v for k, v in g.items() if k != "params"}, params=list(range(i, i + n))))
            i += n
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, state_dict):
        """The inverse of state_dict() on the model's current layout: moments into the flat buffers (the padding between groups stays
        as it is), the step count, and lr / betas / eps of each group by its name."""
        opt = self._state.optimizer
        saved = state_dict["state"]
        steps = set()
        with torch.no_grad():
            for i, (group, cols, shape) in enumerate(self._slots()):
                entry = saved.get(i, saved.get(str(i)))
                if entry is None:      # (torch.optim.Adam has no entry for a parameter it never stepped)
                    continue
                for key, moment in (("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)):
                    src = entry[key]
                    if tuple(src.shape) != tuple(shape):
                        raise ValueError(f"load_state_dict: {key} of parameter {i} is {tuple(src.shape)}, the model has {tuple(shape)}")
                    dst = self._moment_view(moment, group, cols)
                    dst.copy_(src.to(device=dst.device, dtype=torch.float32).reshape(dst.shape))
                steps.add(int(entry["step"]))
        if len(steps) > 1:
            raise ValueError(f"load_state_dict: the parameters carry different step counts {sorted(steps)}; the fused step has one")
        if steps:
            opt.step_count = steps.pop()
        by_name = {g["name"]: g for g in state_dict["param_groups"]}
        for g in self.param_groups:
            src = by_name.get(g["name"])
            if src is not None:
                g.update({k: (tuple(src[k]) if k == "betas" else src[k]) for k in ("lr", "betas", "eps") if k in src})
        self.push()


class GaussianModel:
    """The reference's model class (scene/gaussian_model.py) on one RawTrainState and one DensifyStats; see the module's text."""

    def __init__(self, sh_degree, init_refl_value=1e-3, init_cubemap_resol=128):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.init_refl_value = init_refl_value
        self.env_map_resol = init_cubemap_resol
        self.xyz_scheduler_args = None
        self._state = None          # gsr_train.RawTrainState
        self._stats = None          # gsr_densify.DensifyStats
        self._bound = None          # (pipe, accumulate, async_reflection_tail) of bind()

    # ------------------------------------------------------------------------------------------------ the state and its views
    def _need_state(self, what):
        if self._state is None:
            raise RuntimeError(f"GaussianModel.{what}: the model has no points yet (create_from_pcd, load_ply or restore first)")
        return self._state

    def _need_optimizer(self, what):
        if self.optimizer is None:
            raise RuntimeError(f"GaussianModel.{what} needs training_setup(training_args) first: the model has no optimizer")
        return self._state

    def _adopt(self, state, stats=None):
        """The model goes on with `state` (a fresh one or a successor) and, when given, `stats`: the optimizer object and a bound pipe
        follow, so that nothing renders into or steps a replaced buffer."""
        self._state = state
        if stats is not None:
            self._stats = stats
        if self.optimizer is not None:
            self.optimizer.rebind()
        if self._bound is not None:
            self.bind(self._bound[0], accumulate=self._bound[1], async_reflection_tail=self._bound[2])

    def _raw(self, name):
        return self._state.p[name] if self._state is not None else torch.empty(0)

    def _activated(self, name):
        return self._state.a[name] if self._state is not None else torch.empty(0)

    _xyz = property(lambda self: self._raw("means3D"))
    _opacity = property(lambda self: self._raw("opacities"))
    _scaling = property(lambda self: self._raw("scales"))
    _rotation = property(lambda self: self._raw("rotations"))
    _refl_strength = property(lambda self: self._raw("refl_strengths"))
    get_xyz = property(lambda self: self._raw("means3D"))
    get_features = property(lambda self: self._raw("shs"))
    get_opacity = property(lambda self: self._activated("opacities"))
    get_scaling = property(lambda self: self._activated("scales"))
    get_rotation = property(lambda self: self._activated("rotations"))
    get_refl = property(lambda self: self._activated("refl_strengths"))

    @property
    def _features_dc(self):
        return self._state.p["shs"].detach()[:, :1, :] if self._state is not None else torch.empty(0)

    @property
    def _features_rest(self):
        return self._state.p["shs"].detach()[:, 1:, :] if self._state is not None else torch.empty(0)

    @property
    def env_map(self):
        return None if self._state is None else _Env(self._state.p["cubemap"], self._state.p["fail"])

    get_envmap = env_map

    def get_covariance(self, scaling_modifier=1):
        """The [P, 4, 4] splat-to-world matrices of pipe.compute_cov3D_python (scene/gaussian_model.py:34-40, 153-154), in torch ops: rows
        0-1 the tangent axes times (scale * modifier), row 2 the normal, row 3 the centre; the raw quaternion is normalised inside."""
        xyz, r = self.get_xyz, self._rotation
        s = torch.cat([self.get_scaling * scaling_modifier, torch.ones_like(self.get_scaling)], dim=-1)
        q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        RS = (R * s[:, None, :3]).permute(0, 2, 1)
        P = xyz.shape[0]
        top = torch.cat([RS, torch.zeros((P, 3, 1), dtype=xyz.dtype, device=xyz.device)], dim=2)
        bottom = torch.cat([xyz, torch.ones((P, 1), dtype=xyz.dtype, device=xyz.device)], dim=1)[:, None, :]
        return torch.cat([top, bottom], dim=1)

    # ------------------------------------------------------------------------------------------------ statistics
    def _stat(self, row, column):
        if self._stats is None:
            return torch.empty(0)
        return self._stats.buf[row].unsqueeze(-1) if column else self._stats.buf[row]

    def _set_stat(self, row, value):
        if self._stats is None:
            raise RuntimeError("GaussianModel: the model has no points yet, so no statistics to set")
        self._stats.buf[row].copy_(value.to(self._stats.buf.device).reshape(-1))

    xyz_gradient_accum = property(lambda self: self._stat(0, True), lambda self, v: self._set_stat(0, v))
    denom = property(lambda self: self._stat(1, True), lambda self, v: self._set_stat(1, v))
    accum_w = property(lambda self: self._stat(2, True), lambda self, v: self._set_stat(2, v))
    denom_w = property(lambda self: self._stat(3, True), lambda self, v: self._set_stat(3, v))
    max_radii2D = property(lambda self: self._stat(4, False), lambda self, v: self._set_stat(4, v))

    def add_densification_stats(self, viewspace_point_tensor, update_filter, render_weight, *, radii=None):
        """scene/gaussian_model.py:579-584 in one kernel.  Without `radii`: gsr_densification_stats_filter under the boolean filter;
        max_radii2D is the caller's line (train.py:243).  With `radii` (int32, e.g. render_pkg["radii"]): gsr_densification_stats, which
        selects the rows with radii > 0 and also takes the running maximum, so that line may go; update_filter is then not read."""
        self._need_state("add_densification_stats")
        if radii is not None:
            return self._stats.update(viewspace_point_tensor.grad, radii, render_weight)
        require_entry(lib, "gsr_densification_stats_filter")
        s = self._stats
        P = s.buf.shape[1]
        g = viewspace_point_tensor.grad.float().contiguous()
        f = update_filter.contiguous()
        w = render_weight.float().contiguous()
        if g.shape != (P, 3) or f.dtype != torch.bool or f.numel() != P or w.numel() != P:
            raise ValueError("add_densification_stats: the gradient [P, 3], the bool filter [P] and the weights [P] must match the number of Gaussians")
        with torch.cuda.device(s.buf.device):
            check(lib.gsr_densification_stats_filter(P, ptr(g), ptr(f.view(torch.uint8)), ptr(w), ptr(s.xyz_gradient_accum), ptr(s.denom),
                                                     ptr(s.accum_w), ptr(s.denom_w), stream_ptr(s.buf.device)), "gsr_densification_stats_filter")

    # ------------------------------------------------------------------------------------------------ construction
    def _from_tensors(self, build, tensors, device):
        """A state without a training configuration yet (default learning rates; training_setup replaces it), fresh statistics."""
        self.optimizer = None
        self._state = build(tensors, device, spatial_lr_scale=self.spatial_lr_scale)
        self._stats = gsr_densify.DensifyStats(self._state.p["means3D"].shape[0], self._state.params.flat.device)
        self._adopt(self._state)

    def create_from_pcd(self, pcd, spatial_lr_scale, init_refl_value=1e-3, init_opacity_value=0.1, *, generator=None):
        """scene/gaussian_model.py:160-187 through gsr_init.init_from_point_cloud (3-NN scales, random rotations and cubemap on the GPU)
        and RawTrainState.from_activated.  `pcd`: anything with .points and .colors; `generator`: a torch.Generator on the GPU."""
        import numpy as np
        from gsr_init import init_from_point_cloud
        self.spatial_lr_scale = spatial_lr_scale
        tensors = init_from_point_cloud(np.asarray(pcd.points), np.asarray(pcd.colors), sh_degree=self.max_sh_degree,
                                        init_opacity=init_opacity_value, init_refl=init_refl_value, cubemap_resolution=self.env_map_resol,
                                        generator=generator)
        print("Number of points at initialisation : ", tensors["means3D"].shape[0])
        self._from_tensors(RawTrainState.from_activated, tensors, tensors["means3D"].device)

    def training_setup(self, training_args, *, group=None):
        """scene/gaussian_model.py:189-211: a fresh optimizer (zero moments, step count 0) over the current parameters with the learning
        rates of `training_args` (the keys of gsr_train.DEFAULT_LRS), and zero statistics (max_radii2D stays, as in the reference)."""
        if group is not None:
            raise NotImplementedError("RawTrainState(shard=...): the sharded exchange of the activated copy is not implemented; "
                                      "gsr_adam_act_step takes a range for it")
        old = self._need_state("training_setup")
        self.percent_dense = training_args.percent_dense
        lrs = {k: getattr(training_args, k) for k in DEFAULT_LRS}
        new = RawTrainState({k: v.detach() for k, v in old.p.items()}, old.params.flat.device, spatial_lr_scale=self.spatial_lr_scale, lrs=lrs)
        with torch.no_grad():
            new.optimizer.act.copy_(old.optimizer.act)      # (it may hold what create_from_pcd was given, which is not act(raw) to the bit)
        new.optimizer.frozen = set(old.optimizer.frozen)
        self._stats.buf[:4].zero_()
        self.xyz_scheduler_args = new.xyz_scheduler_args
        self._state = new
        self.optimizer = _Optimizer(self)
        self._adopt(new)

    def load_ply(self, path):
        """scene/gaussian_model.py:296-373 through scene.ply_io.load_ply: the raw tensors and, from the sibling .map, the cubemap."""
        from scene.ply_io import load_ply
        data = load_ply(path, self.max_sh_degree)
        dev = torch.device("cuda", torch.cuda.current_device())
        tensors = {k: torch.tensor(data[k]) for k in _PER_GAUSSIAN}
        if "cubemap" in data:
            self.env_map_resol = int(data["cubemap"].shape[2])
            tensors["cubemap"], tensors["fail"] = torch.tensor(data["cubemap"]), torch.tensor(data["fail"])
        elif self._state is not None:
            tensors["cubemap"], tensors["fail"] = self._state.p["cubemap"].detach(), self._state.p["fail"].detach()
        else:
            raise FileNotFoundError(f"{path.replace('.ply', '.map')}: no environment map beside the PLY and the model has none yet")
        self._from_tensors(RawTrainState, tensors, dev)
        self.active_sh_degree = self.max_sh_degree

    def save_ply(self, path):
        """scene/gaussian_model.py:240-262 through scene.ply_io.save_ply: the raw values, and the environment map beside them."""
        from scene.ply_io import save_ply
        p = self._need_state("save_ply").p
        save_ply(path, p["means3D"], p["shs"], p["opacities"], p["refl_strengths"], p["scales"], p["rotations"], cubemap=p["cubemap"],
                 fail_value=p["fail"])

    def capture(self):
        self._need_optimizer("capture")
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
                self._refl_strength, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(), self.spatial_lr_scale,
                self.env_map_resol)

    def restore(self, model_args, training_args):
        """scene/gaussian_model.py:98-116.  The tuple carries no environment map (the reference's does not either: it restores into a model
        that already has one), so the model keeps its own, or starts a fresh one of env_map_resol."""
        (self.active_sh_degree, xyz, features_dc, features_rest, scaling, rotation, opacity, refl_strength, max_radii2D, xyz_gradient_accum,
         denom, opt_dict, self.spatial_lr_scale, self.env_map_resol) = model_args
        dev = xyz.device
        tensors = dict(means3D=xyz.detach(), shs=torch.cat((features_dc.detach(), features_rest.detach()), dim=1), opacities=opacity.detach(),
                       scales=scaling.detach(), rotations=rotation.detach(), refl_strengths=refl_strength.detach())
        L = self.env_map_resol
        if self._state is not None and self._state.p["cubemap"].shape[2] == L:
            tensors["cubemap"], tensors["fail"] = self._state.p["cubemap"].detach().clone(), self._state.p["fail"].detach().clone()
        else:
            tensors["cubemap"], tensors["fail"] = torch.rand(6, 3, L, L, device=dev) - 0.5, torch.zeros(3, device=dev)
        self._from_tensors(RawTrainState, tensors, dev)
        self.max_radii2D = max_radii2D
        self.training_setup(training_args)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom
        self.optimizer.load_state_dict(opt_dict)

    # ------------------------------------------------------------------------------------------------ schedule
    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def set_opacity_lr(self, lr):
        self._need_optimizer("set_opacity_lr")
        for param_group in self.optimizer.param_groups:
            if param_group["name"] == "opacity":
                param_group["lr"] = lr

    def update_learning_rate(self, iteration):
        self._need_optimizer("update_learning_rate")
        for param_group in self.optimizer.param_groups:
            if param_group["name"] == "xyz":
                lr = self.xyz_scheduler_args(iteration)
                param_group["lr"] = lr
                return lr

    def freeze_xyz(self):
        """scene/gaussian_model.py:213-215: the step leaves positions and rotations, their moments and activated copy bit for bit."""
        self._need_state("freeze_xyz").freeze(("means3D", "rotations"))

    # ------------------------------------------------------------------------------------------------ resets
    def reset_opacity(self, reset_value=0.01, exclusive_msk=None):
        self._need_optimizer("reset_opacity").reset_opacity(reset_value, exclusive_msk=exclusive_msk)

    def reset_refl(self, exclusive_msk=None):
        self._need_optimizer("reset_refl").reset_refl(self.init_refl_value, exclusive_msk=exclusive_msk)

    def reset_scale(self, enlarge_scale=1.5, exclusive_msk=None):
        self._need_optimizer("reset_scale").reset_scale(enlarge_scale, exclusive_msk=exclusive_msk)

    def dist_color(self, noise_range=0.4, exclusive_msk=None, *, noise=None):
        self._need_optimizer("dist_color").dist_color(noise_range, exclusive_msk=exclusive_msk, noise=noise)

    # ------------------------------------------------------------------------------------------------ successor states
    def densify_and_prune(self, max_grad, min_opacity, mean, extent, max_screen_size, *, noise=None, plan="device"):
        """scene/gaussian_model.py:551-577 through gsr_densify.densify_and_prune; returns its `info` (the reference returns nothing)."""
        self._need_optimizer("densify_and_prune")
        self.optimizer.push()
        state, stats, info = gsr_densify.densify_and_prune(self._state, self._stats, max_grad, min_opacity, mean, extent, max_screen_size,
                                                           percent_dense=self.percent_dense, noise=noise, plan=plan)
        self._carry_env_grads(state)
        self._adopt(state, stats)
        return info

    def _carry_env_grads(self, state):
        """The reference leaves the env group alone when it densifies or prunes (cat_tensors_to_optimizer and _prune_optimizer skip it,
        scene/gaussian_model.py:413, 464): the environment map keeps this iteration's gradient and the optimizer step that follows inside
        the same iteration applies it.  A successor state starts with zero gradient slots, so the two env slots are copied over."""
        old = self._state
        side_join(old.params.flat.device)      # (the cubemap gradient may still be in flight on the library's side stream)
        copy_groups(((old.grads.flat, state.grads.flat),), old.params, state.params, [k for k in ("cubemap", "fail") if k in old.params.names])

    def _prune(self, mask):
        if self.optimizer is not None:
            self.optimizer.push()
        state, stats, info = gsr_densify.prune_points(self._state, mask, self._stats)
        self._carry_env_grads(state)
        self._adopt(state, stats)
        return info

    def prune_points(self, mask):
        self._need_optimizer("prune_points")
        return self._prune(mask)

    def prune_points_no_grad(self, mask):
        self._need_state("prune_points_no_grad")
        return self._prune(mask)

    def double_env_map(self):
        self._need_optimizer("double_env_map")
        self.optimizer.push()
        self.env_map_resol = self.env_map_resol * 2
        self._adopt(gsr_envmap.resize_env_map(self._state, self.env_map_resol))

    def filter_env_map(self):
        self._need_optimizer("filter_env_map")
        self._adopt(gsr_envmap.filter_env_map(self._state))

    # ------------------------------------------------------------------------------------------------ the sink-driven step
    def bind(self, pipe, *, accumulate=None, async_reflection_tail=None):
        """Hands the current state's gradient sinks to render() through `pipe`: pipe.gsr_grad_sink, pipe.gsr_reflection_grad_sink and, when
        given, pipe.gsr_accumulate / pipe.gsr_async_reflection_tail.  The model applies it again after every successor state."""
        grads = self._need_state("bind").grads
        pipe.gsr_grad_sink, pipe.gsr_reflection_grad_sink = grads.sink(), grads.sink(("cubemap", "fail"))
        if accumulate is not None:
            pipe.gsr_accumulate = bool(accumulate)
        if async_reflection_tail is not None:
            pipe.gsr_async_reflection_tail = bool(async_reflection_tail)
        self._bound = (pipe, accumulate, async_reflection_tail)
        return pipe
