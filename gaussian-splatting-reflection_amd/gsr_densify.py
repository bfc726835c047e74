"""Adaptive density control on the flat training state (reference: scene/gaussian_model.py:403-584,
train.py:239-255).

The reference prunes / clones / splits by rebuilding every parameter tensor and both Adam moment tensors of every group
once per operation.  Here the masks (a handful of P-sized boolean vectors, evaluated with torch ops) are composed into
one row map per densification step and libgsr_hip.so applies it with one streaming gather per flat buffer
(gsr_gather_rows); the per-view statistics are one fused kernel (gsr_densification_stats) and the split children are
sampled by gsr_split_children.  Ordering of the surviving rows is the reference's: originals, then clones, then the two
copies of the split children, each in index order.

densify_and_prune(..., plan="device") has the library compose the map as well (include/gsr_hip_densify.h: the masks, their ranks and the
last prune as kernels; two 16-byte reads in place of some ten boolean indexes), and prune_points removes rows by a mask with the same
ordered compaction.
"""
import ctypes

import torch

from _gsr import DensifyPlan, GatherGroup, check, lib, ptr, require_entry, stream_ptr
from gsr_train import RawTrainState, copy_groups

PER_GAUSSIAN = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")


class DensifyStats:
    """xyz_gradient_accum, denom, accum_w, denom_w (scene/gaussian_model.py:189-192) and max_radii2D (:183), P floats each."""

    def __init__(self, P, device):
        self.buf = torch.zeros(5, P, dtype=torch.float32, device=device)
        self.xyz_gradient_accum, self.denom, self.accum_w, self.denom_w, self.max_radii2D = self.buf

    def update(self, viewspace_grad, radii, gaussian_weights):
        """train.py:242-245: max_radii2D update + add_densification_stats, one kernel."""
        P = self.buf.shape[1]
        g = viewspace_grad.float().contiguous()
        r = radii.to(torch.int32).contiguous()
        w = gaussian_weights.float().contiguous()
        if g.shape != (P, 3) or r.numel() != P or w.numel() != P:
            raise ValueError("DensifyStats.update: shapes do not match the number of Gaussians")
        with torch.cuda.device(self.buf.device):
            check(lib.gsr_densification_stats(P, ptr(g), ptr(r), ptr(w), ptr(self.xyz_gradient_accum), ptr(self.denom), ptr(self.accum_w),
                                              ptr(self.denom_w), ptr(self.max_radii2D), stream_ptr(self.buf.device)), "gsr_densification_stats")


def _gather(src_flat, dst_flat, row_map, old, new, names):
    groups = (GatherGroup * len(names))()
    for i, k in enumerate(names):
        width = old.slices[k][1] - old.slices[k][0]
        rows_old = old.shapes[k][0]
        groups[i] = GatherGroup(old.slices[k][0], new.slices[k][0], width // rows_old if rows_old else 1)
    n_rows = int(row_map.numel())
    if n_rows == 0:
        return
    with torch.cuda.device(src_flat.device):
        check(lib.gsr_gather_rows(ptr(src_flat), ptr(dst_flat), ptr(row_map), n_rows, groups, len(names), stream_ptr(src_flat.device)),
              "gsr_gather_rows")


def _whole_moments(state, group):
    """Both Adam moment buffers over the WHOLE flat layout.  Unsharded state: the optimizer's own tensors.  Sharded state
    (GaussianTrainState(shard=(rank, N)): the optimizer holds total / N floats, the chunk this rank steps): the chunks of all ranks,
    all-gathered in rank order = buffer order — the row map below addresses rows by their offsets in the whole buffer, and a chunk
    border falls anywhere, also inside a parameter group."""
    import torch.distributed as dist
    opt, total = state.optimizer, state.params.total
    a, b = opt.owned
    if (a, b) == (0, total):
        return opt.exp_avg, opt.exp_avg_sq
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) * (b - a) != total:
        raise RuntimeError("densify_and_prune: the train state is sharded (%r) but there is no process group of that size to gather the Adam "
                           "moments from" % (state.shard,))
    out = []
    for part in (opt.exp_avg, opt.exp_avg_sq):
        if dist.get_backend(group) == "nccl":
            full = torch.empty(total, dtype=part.dtype, device=part.device)
            dist.all_gather_into_tensor(full, part.contiguous(), group=group)
        else:                               # gloo (the CPU-rank rehearsal of the tests): staged through host memory
            host = torch.empty(total, dtype=part.dtype)
            dist.all_gather_into_tensor(host, part.detach().cpu().contiguous(), group=group)
            full = host.to(part.device)
        out.append(full)
    return out[0], out[1]


def _plan_torch(state, stats, max_grad, mean, extent, max_screen_size, percent_dense, N, noise):
    """The plan composed on the host with torch ops: the masks, their composition into the row map and the last prune.  Returns
    (P1, map_param, map_moment, place_children, counts): the two int32 maps gsr_gather_rows takes (map_moment: -1 for clones and
    children), place_children(new) which writes the kept children's positions and scalings into the new store, and the counts of `info`.
    Some ten boolean indexes: each makes the host wait for the device."""
    old = state.params
    dev = old.flat.device
    xyz, scaling, rotation = state.p["means3D"].detach(), state.p["scales"].detach(), state.p["rotations"].detach()
    P0, S = xyz.shape[0], scaling.shape[1]
    # -- a. prune by accumulated blend weight (:549-552)
    accum_w = stats.accum_w / stats.denom_w
    accum_w[stats.denom_w == 0] = 0.0
    idx_a = torch.nonzero(~(accum_w < 0.01), as_tuple=False).flatten()                 # old rows that survive
    grads = (stats.xyz_gradient_accum / stats.denom)[idx_a]                            # :555-556
    grads[grads.isnan()] = 0.0
    max_scale_a = torch.exp(scaling[idx_a]).max(dim=1).values
    # -- b. clone (:536-546): small surfels with a large view-space gradient
    sel_clone = (grads.abs() >= max_grad) & (max_scale_a <= percent_dense * extent)
    clones = idx_a[sel_clone]
    rows_b = torch.cat([idx_a, clones])                                                # old row of each row after the clone step
    # -- c. split (:508-534): large surfels; the clones enter with gradient 0 (padded_grad)
    padded_grad = torch.cat([grads, torch.zeros(clones.numel(), device=dev)])
    max_scale_b = torch.cat([max_scale_a, max_scale_a[sel_clone]])
    sel_split = (padded_grad >= max_grad) & (max_scale_b > percent_dense * extent)
    parents = rows_b[sel_split]                                                        # old rows of the split parents
    k = int(parents.numel())
    child_parent = parents.repeat(N).to(torch.int32)                                   # .repeat(N, 1): copy 1 of all, copy 2 of all
    if noise is None:
        noise = torch.randn(N * k, S, device=dev)
    noise = noise.float().contiguous()
    child_xyz = torch.empty(N * k, 3, device=dev)
    child_scaling = torch.empty(N * k, S, device=dev)
    if k:
        with torch.cuda.device(dev):
            check(lib.gsr_split_children(N * k, S, N, ptr(child_parent), ptr(xyz.contiguous()), ptr(scaling.contiguous()), ptr(rotation.contiguous()),
                                         ptr(noise), ptr(child_xyz), ptr(child_scaling), stream_ptr(dev)), "gsr_split_children")
    rows_c = torch.cat([rows_b[~sel_split], child_parent.long()])                      # after removing the parents (:533-534)
    is_child = torch.cat([torch.zeros(rows_b.numel() - k, dtype=torch.bool, device=dev), torch.ones(N * k, dtype=torch.bool, device=dev)])
    is_new = torch.cat([torch.zeros(idx_a.numel(), dtype=torch.bool, device=dev),
                        torch.ones(clones.numel(), dtype=torch.bool, device=dev)])[~sel_split]
    is_new = torch.cat([is_new, torch.ones(N * k, dtype=torch.bool, device=dev)])       # clones + children: fresh Adam state
    # -- d. prune big points (:559-572).  max_radii2D was reset to zero by densification_postfix (:502), so the
    # screen-size test of the reference can never fire here; it is evaluated on those zeros for fidelity.
    keep = torch.ones(rows_c.numel(), dtype=torch.bool, device=dev)
    if max_screen_size:
        cur_xyz = xyz[rows_c].clone()
        cur_xyz[is_child] = child_xyz
        cur_max_scale = torch.exp(scaling[rows_c]).max(dim=1).values
        cur_max_scale[is_child] = torch.exp(child_scaling).max(dim=1).values if k else cur_max_scale[is_child]
        big_points_vs = torch.zeros_like(keep)
        inside = ((cur_xyz - mean[None].to(dev)) ** 2).sum(dim=-1) < extent ** 2
        big_ws = (cur_max_scale > 0.1 * extent) & inside
        big_ws_far = (cur_max_scale > 1.5 * extent) & ~inside
        keep = ~(big_points_vs | big_ws | big_ws_far)
    final_rows = rows_c[keep]
    P1 = int(final_rows.numel())
    map_param = final_rows.to(torch.int32).contiguous()
    map_moment = torch.where(is_new[keep], torch.full_like(map_param, -1), map_param).contiguous()

    def place_children(new):
        kept_child = is_child[keep]
        if bool(kept_child.any()):
            child_keep = keep[is_child]
            new.p["means3D"][kept_child] = child_xyz[child_keep]
            new.p["scales"][kept_child] = child_scaling[child_keep]
    counts = dict(pruned_by_weight=P0 - int(idx_a.numel()), cloned=int(clones.numel()), split=k, pruned_big=int((~keep).sum()))
    return P1, map_param, map_moment, place_children, counts


def _plan_scratch(P, N, dev):
    """The scratch of the plan entries (include/gsr_hip_densify.h) for P rows and N children per parent, and its size."""
    nbytes = int(lib.gsr_densify_plan_scratch_bytes(P, N))
    if nbytes == 0:
        raise ValueError(f"densification plan: P = {P} rows with N = {N} children per parent is beyond the library's 32-bit positions (P * (N + 1) < 2^31)")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _scatter(src, dst_flat, slot, dst_offset, width):
    """dst rows r with slot[r] >= 0 <- src rows slot[r] (gsr_scatter_rows), one block of `width` floats per row at dst_offset."""
    if slot.numel() == 0 or src.numel() == 0:
        return
    groups = (GatherGroup * 1)(GatherGroup(0, dst_offset, width))
    with torch.cuda.device(dst_flat.device):
        check(lib.gsr_scatter_rows(ptr(src), ptr(dst_flat), ptr(slot), int(slot.numel()), groups, 1, stream_ptr(dst_flat.device)), "gsr_scatter_rows")


def _plan_device(state, stats, max_grad, mean, extent, max_screen_size, percent_dense, N, noise):
    """The same plan composed by libgsr_hip.so (gsr_densify_plan_select / _rows, include/gsr_hip_densify.h): same return values as
    _plan_torch.  Host reads: the 16 bytes of select's counts (they size the children and the maps), and with max_screen_size the 16
    bytes of the rows' counts (the number of rows kept).  No boolean index, no nonzero."""
    for name in ("gsr_densify_plan_select", "gsr_densify_plan_rows", "gsr_scatter_rows"):
        require_entry(lib, name)
    if not max_grad > 0:
        raise ValueError("densify_and_prune(plan='device'): max_grad must be positive (a clone enters the split test with gradient 0)")
    old = state.params
    dev = old.flat.device
    xyz, scaling, rotation = (state.p[k].detach().contiguous() for k in ("means3D", "scales", "rotations"))
    P0, S = xyz.shape[0], scaling.shape[1]
    m = [float(v) for v in mean.detach().reshape(-1).tolist()] if isinstance(mean, torch.Tensor) else [float(v) for v in mean]
    plan = DensifyPlan(max_grad, 0.01, percent_dense * extent, 0.1 * extent, 1.5 * extent, extent ** 2, (ctypes.c_float * 3)(*m),
                       1 if max_screen_size else 0, N, S)
    scratch, nbytes = _plan_scratch(P0, N, dev)
    sel = torch.empty(4, dtype=torch.int32, device=dev)
    parents = torch.empty(P0, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.gsr_densify_plan_select(P0, ctypes.byref(plan), ptr(stats.xyz_gradient_accum), ptr(stats.denom), ptr(stats.accum_w), ptr(stats.denom_w),
                                          ptr(scaling), ptr(scratch), nbytes, ptr(sel), ptr(parents), stream_ptr(dev)), "gsr_densify_plan_select")
    survivors, n_clones, k, _ = sel.tolist()                                            # the one read the children and the maps are sized by
    child_parent = parents[:k].repeat(N)                                                # copy 1 of all, copy 2 of all
    if noise is None:
        noise = torch.randn(N * k, S, device=dev)
    noise = noise.float().contiguous()
    child_xyz = torch.empty(N * k, 3, device=dev)
    child_scaling = torch.empty(N * k, S, device=dev)
    length = survivors - k + n_clones + N * k                                           # of the sequence before the last prune
    maps = torch.empty(3, max(length, 1), dtype=torch.int32, device=dev)
    rows = torch.empty(4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if k:
            check(lib.gsr_split_children(N * k, S, N, ptr(child_parent), ptr(xyz), ptr(scaling), ptr(rotation), ptr(noise), ptr(child_xyz),
                                         ptr(child_scaling), stream_ptr(dev)), "gsr_split_children")
        check(lib.gsr_densify_plan_rows(P0, ctypes.byref(plan), ptr(scratch), nbytes, ptr(xyz), ptr(scaling), ptr(parents), ptr(child_xyz),
                                        ptr(child_scaling), k, ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(rows), stream_ptr(dev)),
              "gsr_densify_plan_rows")
    P1 = rows.tolist()[0] if max_screen_size else length                                # (nothing is dropped without a size threshold)
    map_param, map_moment, child_of = maps[0, :P1], maps[1, :P1], maps[2, :P1]

    def place_children(new):
        _scatter(child_xyz, new.flat, child_of, new.slices["means3D"][0], 3)
        _scatter(child_scaling, new.flat, child_of, new.slices["scales"][0], S)
    counts = dict(pruned_by_weight=P0 - survivors, cloned=n_clones, split=k, pruned_big=length - P1)
    return P1, map_param, map_moment, place_children, counts


def _rebuild(state, group, names, P1, map_param, map_moment, place_children=None):
    """The successor of `state` with P1 rows per per-Gaussian group: parameters gathered by map_param, both Adam moments by map_moment
    (a sharded state: gathered from all ranks, permuted as a whole, re-cut), place_children(new params) for rows that come from
    elsewhere, the other groups copied, a RawTrainState's activated copy refreshed."""
    old = state.params
    dev = old.flat.device
    # -- one gather per flat buffer into a new store of P1 rows
    shapes = {kk: ((P1,) + old.shapes[kk][1:] if kk in names else old.shapes[kk]) for kk in old.names}
    # (the class of the state given: a gsr_train.RawTrainState, whose "scales" are the log-scales read above, stays one; learning rates,
    # step count, betas, eps, frozen groups and the shard are carried over)
    new_state = state.successor(shapes)
    new, opt_new = new_state.params, new_state.optimizer
    old_avg, old_sq = _whole_moments(state, group)
    sharded = opt_new.owned != (0, new.total)
    new_avg = torch.zeros(new.total, dtype=torch.float32, device=dev) if sharded else opt_new.exp_avg
    new_sq = torch.zeros(new.total, dtype=torch.float32, device=dev) if sharded else opt_new.exp_avg_sq
    _gather(old.flat, new.flat, map_param, old, new, names)
    _gather(old_avg, new_avg, map_moment, old, new, names)
    _gather(old_sq, new_sq, map_moment, old, new, names)
    with torch.no_grad():
        if place_children is not None:
            place_children(new)
        # the "env" group is left alone (:462)
        copy_groups(((old.flat, new.flat), (old_avg, new_avg), (old_sq, new_sq)), old, new, [kk for kk in old.names if kk not in names])
        if sharded:                                                                     # this rank's chunk of the new layout
            a2, b2 = opt_new.owned
            opt_new.exp_avg.copy_(new_avg[a2:b2])
            opt_new.exp_avg_sq.copy_(new_sq[a2:b2])
    if isinstance(new_state, RawTrainState):                                            # activated copy of the new rows
        opt_new.activate()
    return new_state


PLANS = {"torch": _plan_torch, "device": _plan_device}


def densify_and_prune(state, stats, max_grad, min_opacity, mean, extent, max_screen_size, percent_dense=0.01, N=2, noise=None, group=None,
                      plan="torch"):
    """GaussianModel.densify_and_prune (scene/gaussian_model.py:548-576) on a GaussianTrainState.  Returns
    (new_state, new_stats, info).  `noise`: optional standard-normal tensor (N*k, scale_dims) for the k split parents (the
    reference draws it with torch.normal); drawn with torch.randn when None.  min_opacity is unused, as in the reference
    (its opacity prune is commented out, :561-562).
    The scales are read as the reference's log-scales.  Given a gsr_train.RawTrainState (whose `p["scales"]` are log-scales) the new state
    is a RawTrainState too: frozen groups and learning rates carried over, the activated copy filled by gsr_activate.
    Sharded state (view-parallel training with gsr_dist.ShardedStep): every rank holds all parameters and, after
    gsr_dist.reduce_densification_stats, the same statistics, so every rank takes the same decisions — given the same `noise`, which the
    caller must then supply (e.g. drawn on rank 0 and broadcast) — and rebuilds the same parameter buffer; the Adam moments, of which a
    rank holds only its chunk, are all-gathered over `group`, permuted as a whole and re-cut into the new layout's chunks.
    plan: who composes the row map.  "torch" (the default): the host, with torch ops (_plan_torch).  "device": libgsr_hip.so
    (_plan_device; include/gsr_hip_densify.h) — the same state bit for bit wherever no max-scale or squared distance lies within a few
    ulp of its threshold (the two plans evaluate expf and the three-term sum separately); it needs max_grad > 0 and takes `mean` as a
    host tensor or a sequence (a device tensor costs one more read).  Everything from the successor state on is shared (_rebuild)."""
    if state.shard is not None and state.shard[1] > 1 and noise is None:
        raise ValueError("densify_and_prune on a sharded state needs `noise` (identical on every rank): ranks drawing their own would split differently")
    if plan not in PLANS:
        raise ValueError(f"densify_and_prune: plan={plan!r}; expected one of {sorted(PLANS)}")
    names = [k for k in PER_GAUSSIAN if k in state.params.names]
    P0 = state.p["means3D"].shape[0]
    P1, map_param, map_moment, place_children, counts = PLANS[plan](state, stats, max_grad, mean, extent, max_screen_size, percent_dense, N, noise)
    new_state = _rebuild(state, group, names, P1, map_param, map_moment, place_children)
    info = dict(counts, before=P0, after=P1)
    return new_state, DensifyStats(P1, state.params.flat.device), info


def prune_points(state, mask, stats=None, group=None):
    """GaussianModel.prune_points / prune_points_no_grad (scene/gaussian_model.py:429-458) on a GaussianTrainState: the rows where `mask`
    (bool, one element per Gaussian) is True go.  Returns (new_state, new_stats, info).  Parameters and both Adam moments of the
    per-Gaussian groups are gathered (no row is new: nothing is zeroed); with `stats` the five statistics rows are carried for the
    remaining points (new_stats is None without); the env group, step count, learning rates, betas, eps, frozen groups and the shard
    carry over; a RawTrainState stays one with its activated copy refreshed.  The ordered map of the remaining rows is built by
    gsr_prune_rows; the host reads its 16 bytes of counts (they size the new store).  A sharded state gathers its moments over `group`,
    as densify_and_prune does."""
    for name in ("gsr_prune_rows", "gsr_densify_plan_scratch_bytes"):
        require_entry(lib, name)
    old = state.params
    dev = old.flat.device
    names = [k for k in PER_GAUSSIAN if k in old.names]
    P0 = state.p["means3D"].shape[0]
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() != 1 or mask.numel() != P0:
        raise ValueError(f"prune_points: mask must be a bool tensor of {P0} elements, one per Gaussian")
    if stats is not None and stats.buf.shape[1] != P0:
        raise ValueError("prune_points: stats do not match the number of Gaussians")
    remove = mask.to(dev).contiguous().view(torch.uint8)
    scratch, nbytes = _plan_scratch(P0, 1, dev)
    row_map = torch.empty(P0, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.gsr_prune_rows(P0, ptr(remove), ptr(scratch), nbytes, ptr(row_map), ptr(counts), stream_ptr(dev)), "gsr_prune_rows")
    P1 = counts.tolist()[0]
    row_map = row_map[:P1]
    new_state = _rebuild(state, group, names, P1, row_map, row_map)
    new_stats = None
    if stats is not None:
        new_stats = DensifyStats(P1, dev)
        if P1:
            groups = (GatherGroup * 5)(*[GatherGroup(r * P0, r * P1, 1) for r in range(5)])
            with torch.cuda.device(dev):
                check(lib.gsr_gather_rows(ptr(stats.buf), ptr(new_stats.buf), ptr(row_map), P1, groups, 5, stream_ptr(dev)), "gsr_gather_rows")
    return new_state, new_stats, dict(pruned=P0 - P1, before=P0, after=P1)
