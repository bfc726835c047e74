"""The environment map's two schedule steps on the flat training state (reference: scene/gaussian_model.py:375-393, train.py:229-230;
CubemapEncoder.resize / CubemapEncoder.filter are the nn.Module forms of the same transforms).

The reference's double_env_map() resamples the cubemap texture to twice its resolution, swaps the new tensor into the `env` group with
both Adam moments of the texture zeroed, and keeps the fail value's moments and the step count; filter_env_map() does the same swap around
a sharpening in sigmoid space.  On the flat state the texture is the `cubemap` slice of one contiguous buffer and `fail` follows it, so a
new resolution is a new layout — built as gsr_densify.densify_and_prune builds its own — and libgsr_hip.so transforms the texture from the
old slice straight into the new one (gsr_envmap_resize, gsr_envmap_sharpen; include/gsr_hip_envmap.h).  Functions take a state and return
the state to go on with.
"""
import torch

import _gsr
from _gsr import check, lib, stream_ptr
from gsr_train import RawTrainState, copy_groups

SHARPEN_CLAMP = (1e-3, 1 - 1e-3)      # cubemap_encoder.py:112 of the reference


def _check_state(state, what):
    if "cubemap" not in state.params.names:
        raise ValueError(f"{what}: the state has no `cubemap` group")
    if state.shard is not None and state.shard[1] > 1:
        # a rank holds only its chunk of the moments, and the chunk borders move with the layout: gsr_densify._whole_moments territory
        raise NotImplementedError(f"{what} on a sharded state (shard=(rank, world_size)) is not implemented")
    _gsr.require_entry(lib, "gsr_envmap_resize")


def resize_env_map(state, new_resolution):
    """CubemapEncoder.resize inside replace_tensor_to_optimizer (scene/gaussian_model.py:375-393) on a GaussianTrainState or a
    RawTrainState: returns a NEW state of the class of the one given whose `cubemap` is [6, C, new_resolution, new_resolution].

      * every group but `cubemap` — parameters, gradient slots and both Adam moments — is copied bit for bit to its new offset (the
        per-Gaussian groups keep theirs, `fail` moves);
      * `cubemap`: the bicubic (align_corners) resample of the old texture, written straight into the new buffer; its gradient slot and
        both moments are zero;
      * spatial_lr_scale, lrs, optimizer.groups (the scheduled means3D rate included), step_count, betas and eps are carried over; for a
        RawTrainState the frozen set too, and the activated buffer is copied bit for bit, not recomputed (it may hold values that are
        not act(raw): RawTrainState.from_activated).

    The reference calls double_env_map() between loss.backward() and optimizer.step(); the step then applies that iteration's gradients
    to every other group and skips the new texture, whose .grad is None.  Here the carried gradient slots do the former and the texture's
    zero gradient on zero moments makes its fused Adam update exactly 0: one optimizer.step() right after this call leaves the texture
    bit for bit and steps everything else as if nothing had happened.

    Every tensor view, gradient sink and `pipe.gsr_*` attribute taken from the old state is stale after the call and must be taken again
    from the new one.  A state without a `cubemap` group or new_resolution < 1: ValueError; a state sharded over more than one rank:
    NotImplementedError."""
    _check_state(state, "resize_env_map")
    new_resolution = int(new_resolution)
    if new_resolution < 1:
        raise ValueError(f"resize_env_map: new_resolution must be at least 1 (got {new_resolution})")
    old = state.params
    dev = old.flat.device
    six, C, L = old.shapes["cubemap"][:3]
    shapes = {k: ((six, C, new_resolution, new_resolution) if k == "cubemap" else old.shapes[k]) for k in old.names}
    new_state = state.successor(shapes)
    new, opt_old, opt_new = new_state.params, state.optimizer, new_state.optimizer
    _gsr.side_join(dev)      # (the old cubemap gradient may still be in flight on the library's side stream: nothing of the old state is freed under it)
    copy_groups(((old.flat, new.flat), (state.grads.flat, new_state.grads.flat), (opt_old.exp_avg, opt_new.exp_avg),
                 (opt_old.exp_avg_sq, opt_new.exp_avg_sq)), old, new, [k for k in old.names if k != "cubemap"], segments=True)
    a, c = old.slices["cubemap"][0], new.slices["cubemap"][0]
    with torch.cuda.device(dev):
        check(lib.gsr_envmap_resize(old.flat.data_ptr() + 4 * a, new.flat.data_ptr() + 4 * c, six * C, L, new_resolution, stream_ptr(dev)),
              "gsr_envmap_resize")
    # (the texture's gradient slot and moments are the zeros the new buffers were made of)
    if isinstance(new_state, RawTrainState):
        with torch.no_grad():
            opt_new.act.copy_(opt_old.act)      # the activated groups lie in front of the texture: one layout for both
    return new_state


def double_env_map(state):
    """gaussians.double_env_map() (train.py:229-230, at iteration == densify_until_iteration): resize_env_map to twice the resolution."""
    _check_state(state, "double_env_map")
    return resize_env_map(state, 2 * state.params.shapes["cubemap"][2])


def filter_env_map(state, factor=2.0):
    """gaussians.filter_env_map() (scene/gaussian_model.py:380-382): the texture becomes
    inverse_sigmoid(adjust_sharpness(sigmoid(texture), factor).clamp(1e-3, 1 - 1e-3)) in one pass and both of its Adam moments are zeroed.
    The layout stays, so the SAME state comes back; the texture's gradient slot and everything else are left alone."""
    _check_state(state, "filter_env_map")
    params, opt = state.params, state.optimizer
    dev = params.flat.device
    six, C, L = params.shapes["cubemap"][:3]
    a, b = params.slices["cubemap"]
    with torch.no_grad():
        tex = params.flat[a:b]
        scratch = torch.empty_like(tex)
        with torch.cuda.device(dev):
            check(lib.gsr_envmap_sharpen(tex.data_ptr(), scratch.data_ptr(), six * C, L, float(factor), SHARPEN_CLAMP[0], SHARPEN_CLAMP[1],
                                         stream_ptr(dev)), "gsr_envmap_sharpen")
        tex.copy_(scratch)
    opt.zero_moments("cubemap")
    return state
