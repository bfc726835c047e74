"""Every entry of the Python surface under the tensor layouts and dtypes a drop-in caller sends.

The reference's loop hands the package transposed camera matrices, a permuted ground-truth image, parameters that are column slices or
offset views of one flat buffer, stride-0 constants.  Every binding turns a tensor into a raw pointer, so a missing `.contiguous()` gives a
wrong image or gradient without an error.  Each test calls an entry (tests/layout_entries.py) once on contiguous float32 clones — the
reference call — and once per layout variant (tests/layouts.py) of ONE tensor argument at a time, then of all arguments together.

Equality rules (layout_entries.compare):
  * forward outputs and deterministic gradients: bit for bit.  Both calls run the same kernels on the same bits once the binding has copied;
  * gradients summed by float atomics (per-Gaussian gradients of both tile backwards, the cubemap / fail-value gradients):
    rel_maxnorm <= 1e-5, the project's bound for "same arithmetic, atomics in another order" (test_sort_drivers_agree_bit_for_bit).
  * layout_entries.reference() runs the reference call twice and holds the repeat to the same rules, so every bound is shown to be
    reachable by the reference alone and everything compared bit for bit is shown to be deterministic.  No tensor needed a wider bound.
  * a gradient that arrives at a non-contiguous leaf has the leaf's shape and dtype, whatever its strides.

The rasterizers and markVisible run under both bindings in one process: the compiled one (csrc/gsr_torch_binding.cpp, loaded at import
when it is built: nothing is built a second time) and ctypes (poison.ctypes_binding()).  tests/test_layouts_host.py is the negative
control: a stride-blind read of every variant differs from the base in most elements and stays inside the parent's storage.

Entries (layout_entries.py; scene "a": P = 2003, 200x120, M = 9 so that SH rows and P * M * 3 * 4 are no multiple of 16 bytes; scene "b":
P = 6000, 301x203 with ragged tile edges, M = 16; cubemap L = 16), each under transposed / column_slice / offset / strided_rows of every
tensor argument, and `expanded` where an argument may be a constant (opacities, reflection strengths, background):
  diff_surfel_rasterization.GaussianRasterizer   shs (a, b), colors_precomp, transMat_precomp; bool env_scope_mask; bg, viewmatrix,
                                                 projmatrix, campos as views; forward + backward; both bindings
  diff_gaussian_rasterization.GaussianRasterizer shs + scales/rotations (antialiasing off, a; on, b), colors_precomp + cov3D_precomp
                                                 (antialiasing on), normals; both bindings
  markVisible                                    both variants, both bindings
  gaussian_renderer                              rasterize_reflect (a, b), deferred_reflection, shading_normal, surface_pass,
                                                 rasterize_eval with and without the environment map; cubemap, fail value, R, T,
                                                 world_view_transform as views
  render(), render(initial_stage), render_fast() with grad, render_fast() under no_grad (fused and initial stage), and all of them on a
                                                 camera object built by the reference's transpositions
  utils.loss_utils                               l1_loss, ssim, l1_loss + ssim on one pair, photometric_loss, normal_consistency_loss with
                                                 and without mask; a cropped render, a permuted ground truth, (1,C,H,W)
  cubemapencoder                                 directions, texture, fail value
  gsr_eval.MetricsTable.image (with and without 8-bit presentation) / .normals, mae_utils.angular_error_map / compute_mae
  utils.image_utils                              psnr, mse, gradient_map, colormap, render_net_image and present_bytes in six modes; the
                                                 refusal of strided `out` / `img_u8` / `error_map` tensors before any device call
  gsr_densify                                    DensifyStats.update; densify_and_prune with `noise` as a view and as float64
  simple_knn.distCUDA2

What the cases exposed, fixed where the pointer is taken: an `shs` input that is a contiguous view at an offset that is no multiple of 16
bytes was refused by the library instead of being copied (both bindings now copy it); surface_pass()'s ray block was built by torch
products of the camera matrices as given, which round differently for the reference's transposed views (surf_normal moved by 7e-6; built
from contiguous copies now); variant G's ctypes forward, both compiled forwards, markVisible and angular_error_map allocated their outputs
before the dtype check.

The dtype contract runs on the same entries: where a binding promises the reference's error, float64 / float16 raise
`expected scalar type Float but found ... for NAME` before anything is allocated on the device; where it converts with `.float()`, the
outputs are those of the call on `.float()` inputs bit for bit and a float64 leaf receives the float32 gradient cast to float64.
"""
import contextlib
import functools
import re

import pytest
import torch

import layouts
import layout_entries as E
from poison import ctypes_binding

pytestmark = pytest.mark.gpu

BOTH_BINDINGS = {**{f"surfel-{f}-{c}": e for (f, c), e in E.SURFEL.items()}, **{f"gauss-{f}-{c}-aa{int(a)}": e for (f, c, a), e in E.GAUSS.items()},
                 **{f"markVisible-{v}": e for v, e in E.MARK_VISIBLE.items()}}
ONE_BINDING = {**{f"rasterize_reflect-{c}": e for c, e in E.FUSED.items()}, **E.PIXEL, **E.EVAL, **E.RENDER, **E.LOSSES, **E.METRICS, **E.SMALL}
ENTRIES = {**BOTH_BINDINGS, **ONE_BINDING}
PLAIN_KINDS = tuple(k for k in layouts.KINDS if k != "expanded")
CASES = [(n, k, b) for n, e in ENTRIES.items() for b in (("compiled", "ctypes") if n in BOTH_BINDINGS else ("default",))
         for k in PLAIN_KINDS + (("expanded",) if e.constant else ())]


@contextlib.contextmanager
def _binding(which):
    import _gsr
    if which == "ctypes":
        with ctypes_binding():
            yield
    else:
        if which == "compiled":
            assert _gsr.PYBIND is not None, "compiled binding not loaded: python gaussian-splatting-reflection_amd/csrc/build.py --binding"
        yield


def _base(name, constants):
    """The entry's contiguous float32 inputs; constants: the inputs of entry.constant are one value repeated (for `expanded`)."""
    e = ENTRIES[name]
    base = dict(e.base())
    if constants:
        for k, value in e.constant.items():
            base[k] = torch.full_like(base[k], value)
    return base


@functools.lru_cache(maxsize=None)
def _reference(name, binding, constants=False):
    with _binding(binding):
        return E.reference(ENTRIES[name], _base(name, constants))


def _clones(base):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}


@pytest.mark.parametrize("name,kind,binding", CASES, ids=[f"{n}-{k}-{b}" for n, k, b in CASES])
def test_layout(name, kind, binding):
    e = ENTRIES[name]
    constants = kind == "expanded"
    base = _base(name, constants)
    ref = _reference(name, binding, constants)
    names = [k for k in (e.constant if constants else e.vary) if layouts.applicable(base[k], kind)]
    assert names, (name, kind)
    with _binding(binding):
        for group in [(k,) for k in names] + [tuple(names)]:
            t = _clones(base)
            for k in group:
                t[k] = layouts.variant(base[k], kind)
                assert torch.equal(t[k], base[k]) and layouts.is_laid_out_differently(t[k])
            out, grads, leaves = E.run(e, t)
            E.compare(e, ref, (out, grads), f"{kind} of {'+'.join(group)}", leaves)


def test_camera_as_the_reference_builds_it():
    """scene/cameras.py: world_view_transform = tensor(getWorld2View2(R, T)).transpose(0, 1), the projection likewise, the full projection
    their product, the camera centre a row of the inverse — render() and render_fast() on such a camera object."""
    for name in ("render", "render_fast"):
        e = ENTRIES[name]
        base = _base(name, False)
        ref = _reference(name, "default")
        t = _clones(base)
        w2v = base["viewmatrix"].t().contiguous()                    # getWorld2View2's matrix; its transpose is the world-view transform
        t["viewmatrix"] = w2v.transpose(0, 1)
        t["projmatrix"] = base["projmatrix"].t().contiguous().transpose(0, 1)
        inv = torch.full((4, 4), layouts.SENTINEL, device="cuda")
        inv[3, :3] = base["campos"]
        t["campos"] = inv[3, :3]
        t["R"] = base["R"].t().contiguous().transpose(0, 1)
        assert not t["viewmatrix"].is_contiguous() and torch.equal(t["viewmatrix"], base["viewmatrix"]) and t["campos"].storage_offset() == 12
        out, grads, leaves = E.run(e, t)
        E.compare(e, ref, (out, grads), "reference camera", leaves)


# ------------------------------------------------------------------------------------------------------------------ losses: the loop's tensors
@pytest.mark.parametrize("which", ["l1", "ssim", "l1+ssim", "photometric"])
def test_losses_on_a_cropped_render_a_permuted_ground_truth_and_a_batch_of_one(which):
    e = E.LOSSES[which]
    base = _base(which, False)
    ref_out, ref_grads = _reference(which, "default")
    img, gt = base["image"], base["gt"]
    C, H, W = img.shape
    gt_hwc = gt.permute(1, 2, 0).contiguous()                      # the loader's HWC array
    # a crop of a larger render, image[:, 3:-5, 7:-2], against the permuted ground truth
    big = torch.full((C, H + 8, W + 9), layouts.SENTINEL, device="cuda")
    big[:, 3:-5, 7:-2] = img
    big.requires_grad_(True)
    crop = big[:, 3:-5, 7:-2]
    assert not crop.is_contiguous() and torch.equal(crop.detach(), img)
    out = e.call({"image": crop, "gt": gt_hwc.permute(2, 0, 1)})
    sum((o * E.upstream(k, o.shape)).sum() for k, o in out.items()).backward()
    for k in ref_out:
        assert E.same_bits(out[k].detach(), ref_out[k]), k
    assert big.grad.shape == big.shape
    assert E.same_bits(big.grad[:, 3:-5, 7:-2], ref_grads["image"])
    outside = big.grad.clone()
    outside[:, 3:-5, 7:-2] = 0
    assert float(outside.abs().max()) == 0.0
    # (1, C, H, W), also as a view
    for kind in (None, "strided_rows", "transposed"):
        x = img.clone() if kind is None else layouts.variant(img, kind)
        leaf = x[None].detach().requires_grad_(True)
        out = e.call({"image": leaf, "gt": gt[None]})
        sum((o * E.upstream(k, o.shape)).sum() for k, o in out.items()).backward()
        for k in ref_out:
            assert E.same_bits(out[k].detach(), ref_out[k]), (k, kind)
        assert leaf.grad.shape == (1, C, H, W) and E.same_bits(leaf.grad[0], ref_grads["image"]), kind


# ------------------------------------------------------------------------------------------------------------------ refusals of strided outputs
def _allocations():
    return torch.cuda.memory_stats()["allocation.all.allocated"]


def test_strided_output_tensors_are_refused_before_any_device_call():
    from gsr_eval import MetricsTable
    from utils import image_utils as iu
    b = _base("metrics-image-q8", False)
    C, H, W = b["image"].shape
    table = MetricsTable(1, b["image"].device)
    rows = table.rows.clone()
    u8 = torch.full((C, H, 2 * W), 7, dtype=torch.uint8, device="cuda")
    ok = torch.zeros((C, H, W), dtype=torch.uint8, device="cuda")
    nb = _base("normal_mae", False)
    emap = torch.full((H, 2 * W), 7.0, device="cuda")
    out = torch.full((H, W, 6), 7, dtype=torch.uint8, device="cuda")
    n = _allocations()
    for kw in (dict(img_u8=u8[:, :, ::2], gt_u8=ok), dict(img_u8=ok, gt_u8=u8[:, :, ::2])):
        with pytest.raises(ValueError, match="contiguous uint8"):
            table.image(0, b["image"], b["gt"], clamp=True, quantize8=True, **kw)
    with pytest.raises(ValueError, match="contiguous float32"):
        table.normals(0, nb["pred"], nb["gt"], error_map=emap[:, ::2])
    with pytest.raises(ValueError, match="contiguous uint8"):
        iu.present_bytes(b["image"], {}, ["RGB"], 0, out=out[:, :, ::2])
    assert _allocations() == n
    torch.cuda.synchronize()
    assert E.same_bits(table.rows, rows) and bool((u8 == 7).all()) and bool((ok == 0).all()) and bool((emap == 7.0).all()) and bool((out == 7).all())


def test_densify_and_prune_with_noise_as_a_view():
    """The split children are sampled from `noise`; the surviving rows, their order and the carried Adam moments are data movement."""
    import numpy as np
    from gsr_densify import DensifyStats, densify_and_prune
    from gsr_train import GaussianTrainState
    P = 3001
    sc = E.S.make_scene(P, "S", seed=7, mu=-3.2)
    tex, fail = E.S.make_cubemap(8, 3, 7)
    tensors = {k: torch.from_numpy(sc[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")}
    tensors["cubemap"], tensors["fail"] = torch.from_numpy(tex), torch.from_numpy(fail)
    st = GaussianTrainState(tensors, "cuda")
    stats = DensifyStats(P, "cuda")
    rs = np.random.RandomState(3)
    denom = rs.randint(0, 5, P).astype(np.float32)
    stats.xyz_gradient_accum.copy_(torch.from_numpy((rs.rand(P) * 8e-4 * denom).astype(np.float32)))
    stats.denom.copy_(torch.from_numpy(denom))
    dw = rs.randint(0, 4, P).astype(np.float32)
    stats.denom_w.copy_(torch.from_numpy(dw))
    stats.accum_w.copy_(torch.from_numpy((rs.rand(P) * 0.05 * dw).astype(np.float32)))
    with torch.no_grad():
        st.p["scales"].copy_(torch.from_numpy(np.log(np.exp(rs.randn(P, 2) * 1.2) * 0.03).astype(np.float32)))
    go = lambda noise: densify_and_prune(st, stats, 0.0002, 0.05, torch.zeros(3), 3.0, None, noise=noise)
    k = go(None)[2]["split"]
    assert k > 10
    noise = torch.from_numpy(rs.randn(2 * k, 2).astype(np.float32)).cuda()
    ref_state, _, ref_info = go(noise.clone())
    again = go(noise.clone())[0]
    assert E.same_bits(again.params.flat, ref_state.params.flat)
    for kind, view in list(layouts.variants_of(noise).items()) + [("float64", noise.double())]:
        state, _, info = go(view)
        assert info == ref_info, kind
        assert E.same_bits(state.params.flat, ref_state.params.flat), kind
        assert E.same_bits(state.optimizer.exp_avg, ref_state.optimizer.exp_avg), kind


# ------------------------------------------------------------------------------------------------------------------ dtype contract
# the name the binding's error gives each argument (the reference's rasterize_points.cu names)
RASTER_NAMES = {"bg": "background", "means3D": "means3D", "shs": "sh", "colors": "colors", "refl_strengths": "refl_strengths", "opacities": "opacity",
                "scales": "scales", "rotations": "rotations", "transmat": "transMat_precomp", "cov3D": "cov3D_precomp", "viewmatrix": "viewmatrix",
                "projmatrix": "projmatrix", "campos": "campos", "normals": "normals"}
RAISING = [(n, b) for n in ("surfel-shs-a", "surfel-colors-a", "surfel-transmat-a", "gauss-shs-a-aa0", "gauss-cov3D-a-aa1", "markVisible-S", "markVisible-G")
           for b in ("compiled", "ctypes")]


def _raises_float(call, name):
    """`call()` raises the reference's dtype error for argument `name`, and has allocated nothing on the device by then."""
    n = _allocations()
    with pytest.raises(RuntimeError, match=r"expected scalar type Float but found \S+ for " + re.escape(name) + r"\b"):
        call()
    assert _allocations() == n, f"{name}: a device allocation precedes the dtype check"


@pytest.mark.parametrize("name,binding", RAISING, ids=[f"{n}-{b}" for n, b in RAISING])
def test_rasterizers_refuse_other_dtypes_before_allocating(name, binding):
    e = ENTRIES[name]
    base = _base(name, False)
    with _binding(binding):
        with torch.no_grad():
            e.call(_clones(base))                                       # warm: the package's one-time allocations are behind us
        for k in e.vary:
            if k not in RASTER_NAMES:
                continue
            for dtype in (torch.float64, torch.float16):
                t = _clones(base)
                t[k] = base[k].to(dtype)
                with torch.no_grad():
                    _raises_float(lambda: e.call(t), RASTER_NAMES[k])
                if k in e.diff:                                         # with autograd on: the same error out of Function.apply
                    t[k] = base[k].to(dtype).requires_grad_(True)
                    _raises_float(lambda: e.call(t), RASTER_NAMES[k])


def test_losses_metrics_and_knn_refuse_other_dtypes_before_allocating():
    from gsr_eval import MetricsTable
    from simple_knn._C import distCUDA2
    from utils import loss_utils as lu
    from utils.mae_utils import angular_error_map
    b = _base("metrics-image", False)
    nb = _base("normal_mae", False)
    pts = _base("distCUDA2", False)["points"]
    table = MetricsTable(1, b["image"].device)
    table.image(0, b["image"], b["gt"])
    table.normals(0, nb["pred"], nb["gt"])
    distCUDA2(pts)
    for dtype in (torch.float64, torch.float16):
        c = {k: v.to(dtype) for k, v in b.items()}
        for fn in (lu.l1_loss, lu.ssim, lu.photometric_loss):
            lu.clear_cache()
            _raises_float(lambda: fn(c["image"], b["gt"]), "img1")
            _raises_float(lambda: fn(b["image"], c["gt"]), "img2")
            _raises_float(lambda: fn(c["image"].requires_grad_(True), b["gt"]), "img1")
        _raises_float(lambda: table.image(0, c["image"], b["gt"]), "img")
        _raises_float(lambda: table.image(0, b["image"], c["gt"]), "gt")
        _raises_float(lambda: table.image(0, b["image"], b["gt"], alpha=c["alpha"]), "alpha")
        _raises_float(lambda: table.image(0, b["image"], b["gt"], gt_mask=c["gt_mask"]), "gt_mask")
        _raises_float(lambda: table.image(0, b["image"], b["gt"], alpha=b["alpha"], background=c["bg"]), "background")
        pred, ngt, other_pts = nb["pred"].to(dtype), nb["gt"].to(dtype), pts.to(dtype)        # (converted out here: the conversion allocates)
        _raises_float(lambda: table.normals(0, pred, nb["gt"]), "pred")
        _raises_float(lambda: table.normals(0, nb["pred"], ngt), "gt")
        _raises_float(lambda: angular_error_map(pred, nb["gt"]), "pred")
        _raises_float(lambda: distCUDA2(other_pts), "points")


CONVERTING = ["deferred_reflection", "shading_normal", "surface_pass", "normal_loss", "normal_loss-masked", "cubemapencoder"]


@pytest.mark.parametrize("name", CONVERTING)
def test_converting_bindings_equal_the_call_on_float_inputs(name):
    """reflection, shading normal, surface pass, normal loss and cubemap encoder convert with .float(): a float64 / float16 input gives the
    outputs of the call on its .float() bit for bit; a float64 LEAF receives a float64 gradient equal to the float32 one cast."""
    e = ENTRIES[name]
    base = _base(name, False)
    for dtype in (torch.float64, torch.float16):
        for group in [(k,) for k in e.converts if k in base] + [tuple(k for k in e.converts if k in base)]:
            other = {k: base[k].to(dtype) for k in group}
            rounded = dict(base, **{k: v.float() for k, v in other.items()})           # float16 rounds the values: the reference sees the same ones
            ref = E.reference(e, rounded) if dtype == torch.float16 else _reference(name, "default")
            t = dict(_clones(base), **other)
            # float16 inputs are not leaves: their gradient would be the float32 one rounded to half, which the atomics bound cannot hold
            frozen = group if dtype == torch.float16 else ()
            out, grads, leaves = E.run(e, t, frozen=frozen)
            ref_grads = {k: g for k, g in ref[1].items() if k not in frozen}
            E.compare(e, (ref[0], ref_grads), (out, grads), f"{dtype} {'+'.join(group)}", leaves)
            for k in group:
                if k in grads:
                    assert grads[k].dtype == dtype == torch.float64, (name, k)
