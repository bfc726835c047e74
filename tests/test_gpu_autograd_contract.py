"""The autograd nodes under the gradient patterns callers send: losses that read a subset of the outputs (the omitted gradients arrive as
None and take the zero-fill or NULL paths of set_materialize_grads(False)), upstream gradients as autograd produces them (stride-0 from
sum() / mean(), strided, permuted, float64), subsets of inputs that require grad, two backward passes through one graph, and inputs
modified between forward and backward.

Nodes: _RasterizeGaussians (variants S and G), _RasterizeReflect, _DeferredReflection, _ShadingNormal, _SurfacePass, _SsimL1, the
normal-loss node and the cubemap encoder, through the entries of tests/layout_entries.py on its small scenes.  Every case is compared with
the same node given explicit, contiguous, float32 upstream gradients, zeros where the case omits one, under the rules of
tests/test_gpu_layouts.py: bit for bit, except gradients summed by float atomics (rel_maxnorm <= 1e-5, layout_entries.ATOMIC_BOUND).
Sums of two backward passes are compared with one backward of the summed loss at rel_maxnorm <= 1e-4
(layout_entries.LINEARITY_BOUND, as test_c3_cull_bit_identity_and_backward_linearity).

Two passes through the fused node with an asynchronous tail.  With async_tail the forward sorts the reflection backward's keys early, into
ctx.scratch.  Reading csrc/gsr_cubemap.hip: ReflTail::carve puts the sorted keys and the pixel list behind the footprint records; the
backward's hipMemsetAsync clears the staging texels and the fail-value slot only, its pixel kernel writes staging, fail slot, footprint
records and the unsorted key slots, and refl_run_combine_kernel reads keys and pixel list as const.  So both survive a backward, and
_gsr.side_hold / side_join only hold references (ctx.scratch keeps the memory alive by itself).  What did not hold: the second pass's
fill and pixel kernel run on the caller's stream and were not ordered behind the first pass's tail, which may still read the footprint
records on the side stream.  _RasterizeReflect.backward now orders the stream behind the tail before it re-uses the scratch; the test pins
that a second pass re-uses the early sort and accumulates exactly the single-pass gradient again.

Frozen environment map.  The fused node wrote the reflection backward's sort keys whenever ANY input required grad; they serve the
cubemap / fail-value gradient alone, so it now writes them only when one of those two requires grad (test_subsets_of_inputs_require_grad).

The loss node _SsimL1 is shared by l1_loss() and ssim() and by design accepts a later pass after autograd released its buffers
(utils/loss_utils.py; tests/test_gpu_loss_edges.py covers that and its in-place check), so "a second backward without retain_graph
raises" is asserted for every node but that one.
"""
import itertools

import pytest
import torch

import layouts
import layout_entries as E
from helpers import rel_maxnorm

pytestmark = pytest.mark.gpu

SURFEL_TAP = E._surfel_entry("shs", "a", tap=True)
GAUSS = E.GAUSS[("shs", "a", False)]
FUSED = E.FUSED["a"]
NODES = {"surfel": SURFEL_TAP, "gauss": GAUSS, "fused": FUSED, "deferred_reflection": E.PIXEL["deferred_reflection"],
         "shading_normal": E.PIXEL["shading_normal"], "surface_pass": E.PIXEL["surface_pass"], "photometric": E.LOSSES["photometric"],
         "normal_loss": E.LOSSES["normal_loss-masked"], "cubemapencoder": E.LOSSES["cubemapencoder"]}


def _subsets(names):
    return [c for r in range(1, len(names) + 1) for c in itertools.combinations(names, r)]


# the differentiable outputs a loss may read, per node
OUTPUT_SUBSETS = {
    "surfel": _subsets(("color", "allmap", "refl_map", "normal_view")),
    "gauss": _subsets(("color", "invdepth", "normal_map", "refl_map")),
    "fused": _subsets(("final", "nworld", "allmap")) + [("refl_color",), ("base",), ("refl_map",)],
    "deferred_reflection": _subsets(("final", "refl_color", "nworld")),
    "surface_pass": _subsets(("surf_depth", "surf_normal")),
}


def _forward(e, frozen=(), base=None):
    base = e.base() if base is None else base
    t = {}
    for k, v in base.items():
        v = v.clone() if torch.is_tensor(v) else v
        t[k] = v.requires_grad_(True) if (torch.is_tensor(v) and k in e.diff and k not in frozen and v.is_floating_point()) else v
    out = e.call(t)
    return t, out


def _diff_outputs(out):
    return {k: o for k, o in out.items() if torch.is_tensor(o) and o.requires_grad}


def _grads(e, t):
    return {k: t[k].grad for k in e.diff if torch.is_tensor(t.get(k)) and t[k].requires_grad}


def _explicit(e, ups, frozen=(), zeros=True):
    """The reference of a case: one backward with explicit contiguous float32 upstream gradients `ups` (name -> tensor), zeros for every
    other differentiable output."""
    t, out = _forward(e, frozen)
    do = _diff_outputs(out)
    gs = {k: (ups[k].float().contiguous() if k in ups else torch.zeros_like(o)) for k, o in do.items() if k in ups or zeros}
    torch.autograd.backward([do[k] for k in gs], [gs[k] for k in gs])
    return {k: o.detach() for k, o in out.items() if torch.is_tensor(o)}, _grads(e, t)


def _check(e, ref, got, what):
    E.compare(e, ref, got, what)


CASES = [(n, s) for n, subsets in OUTPUT_SUBSETS.items() for s in subsets]


@pytest.mark.parametrize("node,subset", CASES, ids=[f"{n}-{'+'.join(s)}" for n, s in CASES])
def test_loss_reads_a_subset_of_the_outputs(node, subset):
    """The omitted gradients arrive as None: zero-fill (rasterizer outputs) or NULL (reflection, surface pass, tap) paths."""
    e = NODES[node]
    t, out = _forward(e)
    do = _diff_outputs(out)
    assert set(subset) <= set(do), (subset, sorted(do))
    ups = {k: E.upstream(k, do[k].shape) for k in subset}
    torch.autograd.backward([do[k] for k in subset], [ups[k] for k in subset])
    got = ({k: o.detach() for k, o in out.items() if torch.is_tensor(o)}, _grads(e, t))
    ref = _explicit(e, ups)
    for k, g in ref[1].items():
        assert g is not None and bool(torch.isfinite(g).all()), k
    _check(e, ref, got, f"subset {subset}")


# ------------------------------------------------------------------------------------------------------------------ upstream gradients as autograd makes them
def _form_loss(form, k, o):
    """(loss term, the explicit upstream gradient it amounts to) for output o."""
    w = E.upstream(k, o.shape)
    if form == "sum":
        return o.sum(), torch.ones_like(o)
    if form == "mean":
        return o.mean(), torch.full_like(o, 1.0 / o.numel())
    if form == "strided":
        idx = (slice(None),) + (slice(None, None, 2),) * (o.dim() - 1)
        g = torch.zeros_like(o)
        g[idx] = 1.0
        return o[idx].sum(), g
    if form == "permuted":
        wp = w.movedim(0, -1).contiguous()               # the loss works on [H,W,C]
        return (o.movedim(0, -1) * wp).sum(), w
    if form == "float64":
        w64 = w.double() * (1.0 + 2.0 ** -30)            # not representable in float32: the node gets its rounding
        return (o.double() * w64).sum(), w64.float()
    raise ValueError(form)


FORMS = ("sum", "mean", "strided", "permuted", "float64")
SCALAR_OUTPUT = ("photometric", "normal_loss")           # a 0-dim loss has nothing to stride or permute
FORM_CASES = [(n, f) for n in sorted(NODES) for f in FORMS if not (n in SCALAR_OUTPUT and f in ("strided", "permuted"))]


@pytest.mark.parametrize("node,form", FORM_CASES, ids=[f"{n}-{f}" for n, f in FORM_CASES])
def test_upstream_gradients_as_autograd_produces_them(node, form):
    e = NODES[node]
    t, out = _forward(e)
    do = _diff_outputs(out)
    terms = {k: _form_loss(form, k, o) for k, o in do.items()}
    loss = None
    for term, _ in terms.values():
        loss = term if loss is None else loss + term
    loss.backward()
    got = ({k: o.detach() for k, o in out.items() if torch.is_tensor(o)}, _grads(e, t))
    ref = _explicit(e, {k: g for k, (_, g) in terms.items()})
    _check(e, ref, got, form)


# ------------------------------------------------------------------------------------------------------------------ subsets of inputs that require grad
def _full_reference(e):
    t, out = _forward(e)
    do = _diff_outputs(out)
    ups = {k: E.upstream(k, o.shape) for k, o in do.items()}
    return ups, _explicit(e, ups)


GRAD_SUBSETS = [(n, c) for n in ("surfel", "gauss", "fused") for c in ("only-opacities", "all-but-shs", "autograd.grad")] + [("fused", "frozen-env")]


@pytest.mark.parametrize("node,case", GRAD_SUBSETS, ids=[f"{n}-{c}" for n, c in GRAD_SUBSETS])
def test_subsets_of_inputs_require_grad(node, case):
    """frozen-env: cubemap and fail value frozen, as in the reference's initial stage — the fused node then writes no sort keys and still
    returns the per-Gaussian gradients."""
    e = NODES[node]
    ups, ref = _full_reference(e)
    names = [k for k in e.diff if k in e.base()]
    if case == "autograd.grad":
        t, out = _forward(e)
        do = _diff_outputs(out)
        chosen = [k for k in ("opacities", "scales", "cubemap") if k in names]
        res = torch.autograd.grad([do[k] for k in ups], [t[k] for k in chosen], [ups[k] for k in ups])
        assert all(t[k].grad is None for k in names)           # autograd.grad leaves every .grad alone
        _check(e, (ref[0], {k: ref[1][k] for k in chosen}), ({k: o.detach() for k, o in out.items() if torch.is_tensor(o)}, dict(zip(chosen, res))), case)
        return
    frozen = {"only-opacities": [k for k in names if k != "opacities"], "all-but-shs": ["shs"], "frozen-env": ["cubemap", "fail"]}[case]
    t, out = _forward(e, frozen)
    if case == "frozen-env":
        fn = out["final"].grad_fn
        assert fn.sort_keys is None and fn.scratch is None          # no sort keys for a gradient nobody takes
    do = _diff_outputs(out)
    torch.autograd.backward([do[k] for k in ups], [ups[k] for k in ups])
    assert all(t[k].grad is None for k in frozen)
    live = [k for k in names if k not in frozen]
    assert live
    _check(e, (ref[0], {k: ref[1][k] for k in live}), ({k: o.detach() for k, o in out.items() if torch.is_tensor(o)}, {k: t[k].grad for k in live}), case)


@pytest.mark.parametrize("node", sorted(NODES))
def test_nothing_requires_grad_keeps_no_backward_state(node):
    e = NODES[node]
    with torch.no_grad():
        _, plain = _forward(e, frozen=e.diff)
    with torch.enable_grad():
        t, out = _forward(e, frozen=e.diff)
    for k, o in out.items():
        if torch.is_tensor(o):
            assert o.grad_fn is None and not o.requires_grad, k
            assert E.same_bits(o, plain[k]), k


# ------------------------------------------------------------------------------------------------------------------ two passes through one graph
TWO_PASS = [n for n in sorted(NODES) if n != "fused"]


def _two_upstreams(do):
    g1 = {k: E.upstream(k, o.shape) for k, o in do.items()}
    g2 = {k: E.upstream(k + "#2", o.shape) for k, o in do.items()}
    return g1, g2


@pytest.mark.parametrize("node", TWO_PASS)
def test_two_backward_passes_through_one_graph(node):
    e = NODES[node]
    t, out = _forward(e)
    do = _diff_outputs(out)
    g1, g2 = _two_upstreams(do)
    outs = [do[k] for k in g1]
    # the same loss twice: exactly twice the single-pass gradient (to the atomics bound where atomics sum it)
    single = _explicit(e, g1)
    torch.autograd.backward(outs, [g1[k] for k in g1], retain_graph=True)
    torch.autograd.backward(outs, [g1[k] for k in g1], retain_graph=True)
    twice = {k: (None if g is None else 2.0 * g) for k, g in single[1].items()}
    _check(e, (single[0], twice), ({k: o.detach() for k, o in out.items() if torch.is_tensor(o)}, _grads(e, t)), "same loss twice")
    # two different losses, one after the other, against one backward of their sum
    t, out = _forward(e)
    do = _diff_outputs(out)
    outs = [do[k] for k in g1]
    torch.autograd.backward(outs, [g1[k] for k in g1], retain_graph=True)
    torch.autograd.backward(outs, [g2[k] for k in g1])
    summed = _explicit(e, {k: g1[k] + g2[k] for k in g1})
    for k, r in summed[1].items():
        err = rel_maxnorm(t[k].grad.double().cpu().numpy(), r.double().cpu().numpy())
        assert err <= E.LINEARITY_BOUND, (node, k, err)
    if node == "photometric":
        return          # the shared loss node accepts a later pass by design (module docstring)
    # a further pass without retain_graph: autograd's own error, and every .grad as it was
    before = {k: g.clone() for k, g in _grads(e, t).items()}
    with pytest.raises(RuntimeError, match="backward through the graph a second time|already been freed"):
        torch.autograd.backward(outs, [g1[k] for k in g1])
    for k, g in before.items():
        assert E.same_bits(t[k].grad, g), k


PARAMS8 = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths", "cubemap", "fail")
SINKS = [(False, False, False), (True, False, False), (False, True, False), (True, True, False), (False, True, True), (True, True, True)]


@pytest.mark.parametrize("raster_sink,refl_sink,async_tail", SINKS, ids=[f"raster{int(a)}-refl{int(b)}-async{int(c)}" for a, b, c in SINKS])
def test_two_backward_passes_through_the_fused_node(raster_sink, refl_sink, async_tail):
    """All four combinations of the two gradient sinks, and the asynchronous tail whose early key sort has filled ctx.scratch (module
    docstring).  Every gradient lands in one flat buffer: through its sink (accumulate mode) or through autograd, whose .grad are views
    of the same buffer."""
    import _gsr
    from gsr_dist import FlatGrads
    e = FUSED
    base = e.base()
    outs_read = ("final", "allmap")
    g1 = {k: E.upstream(k, s) for k, s in (("final", (3, 120, 200)), ("allmap", (8, 120, 200)))}
    g2 = {k: E.upstream(k + "#2", v.shape) for k, v in g1.items()}
    single = _explicit(e, g1, zeros=False)
    summed = _explicit(e, {k: g1[k] + g2[k] for k in g1}, zeros=False)

    def two_passes(second):
        t = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
        leaves = {k: t[k].requires_grad_(True) for k in PARAMS8}
        t["means2D"].requires_grad_(True)
        fg = FlatGrads(leaves)
        t["_sinks"] = (fg.sink() if raster_sink else None, fg.sink(names=("cubemap", "fail")) if refl_sink else None, True, async_tail)
        out = e.call(t)
        fn = out["final"].grad_fn
        assert fn.sort_keys is not None and (fn.scratch is not None) == async_tail
        outs = [out[k] for k in outs_read]
        torch.autograd.backward(outs, [g1[k] for k in outs_read], retain_graph=True)
        torch.autograd.backward(outs, [second[k] for k in outs_read], retain_graph=True)
        assert fn.passes == 2
        _gsr.side_join()
        torch.cuda.synchronize()
        got = {k: fg.view(k).clone() for k in PARAMS8}
        got["means2D"] = t["means2D"].grad.clone()
        # a third pass without retain_graph would need the freed buffers only after this one: release them, then autograd refuses
        torch.autograd.backward(outs, [g1[k] for k in outs_read])
        _gsr.side_join()
        with pytest.raises(RuntimeError, match="backward through the graph a second time|already been freed"):
            torch.autograd.backward(outs, [g1[k] for k in outs_read])
        return got

    got = two_passes(g1)
    for k, g in got.items():
        r = 2.0 * single[1][k]
        err = rel_maxnorm(g.double().cpu().numpy(), r.double().cpu().numpy())
        assert bool(torch.isfinite(g).all()) and err <= E.ATOMIC_BOUND, ("same loss twice", k, err)
    got = two_passes(g2)
    for k, g in got.items():
        err = rel_maxnorm(g.double().cpu().numpy(), summed[1][k].double().cpu().numpy())
        assert err <= E.LINEARITY_BOUND, ("two losses", k, err)


# ------------------------------------------------------------------------------------------------------------------ in-place modification
# the inputs each node saves for its backward (variant S does not save the opacities, as the reference; the encoder not the fail value)
SAVED = {"surfel": ("means3D", "shs", "refl_strengths", "scales", "rotations"),
         "gauss": ("means3D", "shs", "refl_strengths", "scales", "rotations", "normals", "opacities"),
         "fused": ("means3D", "shs", "refl_strengths", "scales", "rotations", "cubemap", "fail"),
         "deferred_reflection": ("normal_view", "base_color", "refl_map", "cubemap", "fail"), "shading_normal": ("normal_view",),
         "surface_pass": ("allmap",), "normal_loss": ("rend_normal", "surf_normal"), "cubemapencoder": ("dirs", "cubemap")}
INPLACE = [(n, k) for n, names in SAVED.items() for k in names]


@pytest.mark.parametrize("node,name", INPLACE, ids=[f"{n}-{k}" for n, k in INPLACE])
def test_saved_input_modified_in_place_raises(node, name):
    e = NODES[node]
    t, out = _forward(e)
    do = _diff_outputs(out)
    with torch.no_grad():
        t[name].mul_(1.0)               # same values, another version
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.backward(list(do.values()), [E.upstream(k, o.shape) for k, o in do.items()])
    assert all(g is None for g in _grads(e, t).values())


# inputs the binding converts (.float().contiguous()): given as a view, the node saves a private contiguous copy
PRIVATE = [(n, k) for n in ("deferred_reflection", "shading_normal", "surface_pass", "normal_loss", "cubemapencoder") for k in SAVED[n]]
PRIVATE += [("fused", "cubemap"), ("fused", "fail")]


@pytest.mark.parametrize("node,name", PRIVATE, ids=[f"{n}-{k}" for n, k in PRIVATE])
def test_view_input_modified_in_place_gives_the_gradient_at_the_forwards_values(node, name):
    e = NODES[node]
    ups, ref = _full_reference(e)
    base = dict(e.base())
    kind = "strided_rows" if layouts.applicable(base[name], "strided_rows") else "column_slice"
    base[name] = layouts.variant(base[name], kind)
    t = {}
    for k, v in base.items():
        v = v if k == name or not torch.is_tensor(v) else v.clone()
        t[k] = v.detach().requires_grad_(True) if (torch.is_tensor(v) and k in e.diff and v.is_floating_point()) else v
    assert not t[name].is_contiguous()
    out = e.call(t)
    do = _diff_outputs(out)
    with torch.no_grad():
        t[name].add_(0.5)               # other values: a backward that read this tensor again would differentiate somewhere else
    torch.autograd.backward([do[k] for k in ups], [ups[k] for k in ups])
    _check(e, ref, ({k: o.detach() for k, o in out.items() if torch.is_tensor(o)}, _grads(e, t)), f"{name} modified after the forward")
