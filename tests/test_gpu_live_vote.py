"""GPU: the forward tile kernels vote against the bounding box of the block's pixels that are still alive (LiveBox, csrc/gsr_tile_walk.hpp),
and that changes no bit of any result.  A retired pixel never blends again, so an entry that only reaches retired pixels is an empty pair
with or without the vote; the reference of every case is the same call with per-wave culling off ("cull" = 0: every list entry is
evaluated), compared with torch.equal on every tensor the forward returns, num_rendered and everything the backward reads from the forward:
the per-pixel state it starts from (n_contrib, final_T) and the batches' blend masks, word for word (where no pair grazes: see _raster).

The parameter gradients of a backward with fixed upstream gradients cannot be held to torch.equal: they are sums of float atomics, whose
order changes from run to run, and on every one of these scenes two runs of the SAME call already differ in every gradient tensor (culling
off against itself, four runs each, measured on the MI355X; at C3 two builds differ by 3e-7 of a gradient's largest element).  With the
backward's inputs equal word for word, the order of the additions is all that can differ, so each gradient is held to the reference's own
spread: the reference runs twice, and the run with culling on may be no further from the first reference run than 8 times the second
one is (largest element-wise difference), where a spread below 8 ulp of the tensor's largest element counts as 8 ulp: the two reference
runs agree on some tensors in some runs, and one reordered sum moves its element by a few ulp of its largest partial sum.  That is at most
7.6e-6 of the largest element, against the 5e-5 to which tests/test_gpu_parity.py::test_cull_is_bit_exact holds the same comparison.
_assert_same prints each figure.

The scenes (tests/live_vote_scenes.py; tests/test_live_vote_scenes.py holds each to 25 % of its pixels retired before their list ends by the
oracle) run at 40x24 and 41x23 px on every instance of the kernels: the rasterizers of both variants (training, no reflection), render()
(training with the reflection epilogue, and without it in the initial stage) and render_fast() under no_grad (inference, both stages).
The development counter (gsr_set_option "dev" bits 2 and 4) gives the evaluated pairs with the live box and with the whole-block vote."""
import numpy as np
import pytest
import torch

import live_vote_scenes as L
from helpers import HipGauss, HipSurfel, S, to_cuda
from test_gpu_dropin import _Pipe, _model, _view

pytestmark = pytest.mark.gpu

SIZE_IDS = ["%dx%d" % s for s in L.SIZES]


def _each_cull(run, culls=(0, 1)):
    """run() with culling off, then on (culls = (0, 0, 1): the reference twice, for the spread of its gradients)."""
    import _gsr
    res = []
    try:
        for cull in culls:
            _gsr.set_option("cull", cull)
            res.append(run())
            torch.cuda.synchronize()
    finally:
        _gsr.set_option("cull", 1)
    return res


def _assert_same(ref, got, what, again=None):
    """Every entry of `got` equal to `ref`'s; gradients (dL_*, grad_*) within the spread between `ref` and `again`, the reference's second run."""
    assert ref.keys() == got.keys(), what
    for k in ref:
        if ref[k] is None or got[k] is None:
            assert ref[k] is None and got[k] is None, (what, k)
        elif k.startswith(("dL_", "grad_")):
            assert ref[k].shape == got[k].shape == again[k].shape, (what, k)
            if ref[k].numel() == 0:
                continue
            d, spread = float((got[k] - ref[k]).abs().max()), float((again[k] - ref[k]).abs().max())
            floor = 8 * float(ref[k].abs().max()) * 2.0 ** -23
            print("%s %s: culling on differs from the reference by %.3g, the reference from itself by %.3g (8 ulp of its largest element: %.3g)" % (what, k, d, spread, floor))
            assert d <= 8 * max(spread, floor), (what, k, d, spread, floor)
        elif isinstance(ref[k], torch.Tensor):
            assert ref[k].shape == got[k].shape and torch.equal(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()))
        else:
            assert ref[k] == got[k], (what, k, ref[k], got[k])


def _raster(variant, kw, masks=True, backward=True):
    """The rasterizer of `variant`: outputs, per-pixel state, blend masks and gradients as tensors.  masks = False leaves the blend masks
    out: a pair in which some lane's ray grazes the splat plane is forced into the mask of its batch for the backward to look at, whether
    it blended or not, and a culled pair is never seen to graze; the backward drops it again, so the gradients are still compared."""
    import _gsr
    H, W = kw["image_height"], kw["image_width"]
    g = S.make_upstream_grads(H, W, 5)
    hip = HipSurfel(kw, requires_grad=backward) if variant == "S" else HipGauss(kw, requires_grad=backward, antialiasing=bool(W % 2))
    if variant == "S":
        out = dict(color=hip.color, radii=hip.radii, allmap=hip.allmap, refl_strength_map=hip.refl_map, gaussian_weights=hip.gw)
    else:
        out = dict(color=hip.color, radii=hip.radii, invdepth=hip.invdepth, normal_map=hip.normal_map, refl_strength_map=hip.refl_map)
    out = {k: v.detach().clone() for k, v in out.items()}
    if not backward:
        return out
    out["num_rendered"] = hip.R
    for k in ("n_contrib", "final_T"):
        out[k] = torch.from_numpy(hip.state(k))
    if masks and hip.R > 0:
        geom, binning, img = hip.ctx.saved_tensors[-3:]
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        out["blend_mask"] = _gsr.debug_fetch(0 if variant == "S" else 1, "blend_mask", hip.P, hip.R, W, H, geom, binning, img, torch.int64,
                                             (16 * (hip.R // 64 + tiles + 1),))
    gh = hip.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"]) if variant == "S" else hip.backward(g["dL_dcolor"], g["dL_dinvdepth"],
                                                                                                         g["dL_dnormal"], g["dL_drefl"])
    for k, v in gh.items():
        out[k] = None if v is None else torch.from_numpy(v)
    return out


def _blending_pairs(variant, mask):
    """(wave, entry) pairs that blended into at least one pixel, from a forward's blend masks (no forced entries in the scene)."""
    m = mask.cpu().numpy().view(np.uint64)
    if variant == "S":
        m = np.bitwise_or.reduce(m.reshape(-1, 4, 4), axis=2)      # [batch][quadrant][4x4 sub-block] -> per 8x8 block
    else:
        m = m[:len(m) // 4]
    return int(np.unpackbits(m.reshape(-1).view(np.uint8)).sum())


def _pairs():
    import _gsr
    e = torch.empty(0, device="cuda")
    torch.cuda.synchronize()
    return int(_gsr.debug_fetch(0, "pairs", 0, 0, 16, 16, e, e, e, torch.int64, (1,)).item())


def _model_and_view(kw, requires_grad):
    from cubemapencoder import CubemapEncoder
    W, H = kw["image_width"], kw["image_height"]
    t = to_cuda(kw)
    leaves = {k: t[k].clone().requires_grad_(requires_grad) for k in ("means3D", "opacities", "scales", "rotations", "shs", "refl_strengths")}
    tex, fail = S.make_cubemap(16, 3, 3)
    env = CubemapEncoder(output_dim=3, resolution=16).cuda()
    with torch.no_grad():
        env.params["Cubemap_texture"].copy_(torch.from_numpy(tex))
        env.params["Cubemap_failv"].copy_(torch.from_numpy(fail) + 0.25)
    return leaves, env, _model(leaves, env, degree=kw["sh_degree"]), _view(S.make_camera(W, H), W, H), t["bg"]


def _render(kw, initial_stage):
    """render(): every tensor it returns, and the gradients of the parameters and the cubemap under fixed upstream gradients."""
    from gaussian_renderer import render
    leaves, env, PC, View, bg = _model_and_view(kw, True)
    pkg = render(View, PC, _Pipe, bg, initial_stage=initial_stage)
    out = {k: v.detach().clone() for k, v in pkg.items() if isinstance(v, torch.Tensor)}
    gen = torch.Generator(device="cpu").manual_seed(11)
    loss = 0.0
    for k in sorted(pkg):
        v = pkg[k]
        if isinstance(v, torch.Tensor) and v.requires_grad and k != "viewspace_points":
            loss = loss + (v * (torch.randn(v.shape, generator=gen) / v[0].numel()).cuda()).sum()
    loss.backward()
    for k, v in leaves.items():
        out["grad_" + k] = v.grad
    out["grad_viewspace_points"] = pkg["viewspace_points"].grad
    if not initial_stage:
        for k, v in env.params.items():
            out["grad_" + k] = v.grad
    return out


def _render_fast(kw, initial_stage):
    from gaussian_renderer import render_fast
    leaves, env, PC, View, bg = _model_and_view(kw, False)
    with torch.no_grad():
        pkg = render_fast(View, PC, _Pipe, bg, initial_stage=initial_stage)
    return {k: v.clone() for k, v in pkg.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("size", L.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name", L.NAMES)
def test_rasterizer_is_bit_identical(name, size, variant):
    kw = L.scene(name, variant, *size)
    ref, again, got = _each_cull(lambda: _raster(variant, kw, masks=name != "rare"), (0, 0, 1))
    assert ref["num_rendered"] > 0
    _assert_same(ref, got, (name, size, variant), again)


@pytest.mark.parametrize("initial_stage", [False, True], ids=["reflect", "initial"])
@pytest.mark.parametrize("size", L.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name", L.NAMES)
def test_render_is_bit_identical(name, size, initial_stage):
    kw = L.scene(name, "S", *size)
    ref, again, got = _each_cull(lambda: _render(kw, initial_stage), (0, 0, 1))
    assert float(ref["rend_alpha"].max()) > 0.5
    _assert_same(ref, got, (name, size, initial_stage), again)


@pytest.mark.parametrize("initial_stage", [False, True], ids=["reflect", "initial"])
@pytest.mark.parametrize("size", L.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name", L.NAMES)
def test_render_fast_under_no_grad_is_bit_identical(name, size, initial_stage):
    kw = L.scene(name, "S", *size)
    ref, got = _each_cull(lambda: _render_fast(kw, initial_stage))
    assert float(ref["rend_alpha"].max()) > 0.5
    _assert_same(ref, got, (name, size, initial_stage))


@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("size", L.SIZES, ids=SIZE_IDS)
def test_empty_scene(size, variant):
    """P = 0: no list to walk."""
    kw = L.empty(variant, *size)
    ref, got = _each_cull(lambda: _raster(variant, kw, backward=False))
    _assert_same(ref, got, ("empty", size, variant))
    if variant == "S":
        ref, got = _each_cull(lambda: _render_fast(kw, False))
        _assert_same(ref, got, ("empty render_fast", size))


@pytest.mark.parametrize("variant", ["S", "G"])
@pytest.mark.parametrize("size", L.SIZES, ids=SIZE_IDS)
def test_live_box_evaluates_fewer_pairs(size, variant):
    """`stack` (pixels retire inside the first batches of lists of more than 130 entries): the pairs the forward evaluates with the live box
    are strictly fewer than with the vote against the whole block, and no fewer than the pairs that blend."""
    import _gsr
    kw = L.scene("stack", variant, *size)
    count = {}
    try:
        for what, dev in (("live", 2), ("block", 6)):
            _gsr.set_option("dev", dev)
            before = _pairs()
            out = _raster(variant, kw)
            count[what] = _pairs() - before
    finally:
        _gsr.set_option("dev", 0)
    before = _pairs()
    plain = _raster(variant, kw)
    assert _pairs() == before                    # the counter only runs under the development option
    blending = _blending_pairs(variant, plain["blend_mask"])
    print("%s %dx%d: %d pairs evaluated against the whole block, %d against the live box, %d blend" % ((variant,) + size + (count["block"], count["live"], blending)))
    assert blending > 0
    assert blending <= count["live"] < count["block"]
    forward = lambda r: {k: v for k, v in r.items() if not k.startswith("dL_")}
    _assert_same(forward(plain), forward(out), "counting instance against the production instance")
