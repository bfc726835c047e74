"""A refused workspace allocation fails cleanly and leaves nothing behind.

The refusal is INJECTED (a callback that answers NULL, an allocation patched to raise): no test exhausts device memory or caps the allocator.
One small scene (3000 surfels / Gaussians, 200x136 = ragged tiles, cubemap 16; tests/test_gpu_render_options.py's sizes and seed).

Through the C ABI (ctypes, a test-owned gsr_alloc_fn that allocates with torch and returns NULL for one chosen buffer) every forward entry
must answer GSR_E_ALLOC with the byte count in its message, the kernels it had already enqueued must finish (torch.cuda.synchronize()
returns, no sticky error), gsr_side_join must return 0, and the next call of the same thread on the same stream must compute what the call
before the refusal computed, bit for bit, and what the oracle computes, under tests/test_gpu_parity.py's bars.

Through Python the n-th request of _gsr.Workspace raises a torch.OutOfMemoryError the test created: that very object must reach the caller
of GaussianRasterizer (both variants), rasterize_reflect, rasterize_eval, render and render_fast; nothing may stay in _gsr._side_held, and
the next call must match the run before the refusal.

The oracle's forward and backward of each variant are computed once and shared; every tolerance is tests/test_gpu_parity.py's
(_run_surfel / _run_gauss), and the bound of the fused step after the async-sort refusal is the suite's bound for the same arithmetic with
its atomics in another order (rel_maxnorm <= 1e-5, tests/test_gpu_layouts.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import GATE_BUDGET, HipGauss, HipSurfel, S, assert_image_close, grad_gate, n_contrib_ok, psnr, rel_maxnorm, scene_kwargs, to_cuda
from poison import ctypes_binding
from test_gpu_dropin import _Pipe, _model, _view

pytestmark = pytest.mark.gpu

P, W, H, L, SEED, MU = 3000, 200, 136, 16, 5, -2.8
BG = (0.1, 0.2, 0.3)
GRAD_TOL, PSNR_MIN = 1e-4, 50.0
GSR_E_ALLOC = -3
GEOM, BINNING, IMAGE = 0, 1, 2
OOM = getattr(torch, "OutOfMemoryError", None) or torch.cuda.OutOfMemoryError


# ------------------------------------------------------------------------------------------------ the scene and its oracle, computed once
@functools.lru_cache(maxsize=None)
def _scene(variant):
    """(kwargs as numpy, the same on the device, camera): never modified."""
    kw, cam, _ = scene_kwargs(variant, P, W, H, SEED, MU, 3, BG)
    return kw, to_cuda(kw), cam


@functools.lru_cache(maxsize=None)
def _oracle(variant):
    """The oracle's forward, the integer state the tests compare exactly, and its backward for make_upstream_grads(SEED)."""
    from oracle import oracle as orc
    kw = _scene(variant)[0]
    g = S.make_upstream_grads(H, W, SEED)
    if variant == "S":
        o = orc.SurfelOracle(np.float32)
        ref = o.forward(**kw)
        gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dallmap=g["dL_dplanes"], dL_drefl_strength_map=g["dL_drefl"])
    else:
        o = orc.GaussOracle(np.float32)
        ref = o.forward(antialiasing=True, **kw)
        gr = o.backward(dL_dcolor=g["dL_dcolor"], dL_dinvdepth=g["dL_dinvdepth"], dL_dnormal_map=g["dL_dnormal"], dL_drefl_strength_map=g["dL_drefl"])
    state = {k: o.state(k) for k in ("point_list", "ranges", "n_contrib")}
    return ref, state, gr, g


@functools.lru_cache(maxsize=None)
def _reflection():
    """Cubemap, fail value and the camera block of the fused reflection epilogue, on the device."""
    import gaussian_renderer as GR
    tex, fail = S.make_cubemap(L, 3, SEED)
    view = _view(_scene("S")[2], W, H)
    cam = GR._cam_block(view.world_view_transform, view.HWK, view.R, view.T)
    return torch.from_numpy(tex).cuda(), torch.from_numpy(fail + np.float32(0.25)).cuda(), cam, view


def _check_rasterizer_against_oracle(variant, hip):
    """tests/test_gpu_parity.py::_run_surfel / _run_gauss on a finished HipSurfel / HipGauss forward: integers exact, images and gradients
    under their bars."""
    ref, state, gr, g = _oracle(variant)
    out = hip.out()
    assert out["num_rendered"] == ref["num_rendered"]
    np.testing.assert_array_equal(out["radii"], ref["radii"])
    np.testing.assert_array_equal(hip.state("point_list").astype(np.uint32), state["point_list"])
    np.testing.assert_array_equal(hip.state("ranges").astype(np.uint32), state["ranges"])
    nc = hip.state("n_contrib").astype(np.uint32)
    if variant == "S":
        assert n_contrib_ok(nc[0], state["n_contrib"][0]) and n_contrib_ok(nc[1], state["n_contrib"][1])
        assert psnr(out["color"], ref["color"]) >= PSNR_MIN
        assert_image_close(out["color"], ref["color"], 3e-5)
        assert psnr(out["refl_strength_map"], ref["refl_strength_map"]) >= PSNR_MIN
        for plane in range(8):
            scale = max(1.0, float(np.abs(ref["allmap"][plane]).max()))
            assert psnr(out["allmap"][plane], ref["allmap"][plane], peak=scale) >= PSNR_MIN, plane
        gh = hip.backward(g["dL_dcolor"], g["dL_dplanes"], g["dL_drefl"])
        names = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_drefl_strengths", "dL_dscales", "dL_drotations")
    else:
        assert n_contrib_ok(nc[0], state["n_contrib"])
        for k in ("color", "normal_map", "refl_strength_map", "invdepth"):
            scale = max(1.0, float(np.abs(ref[k]).max()))
            assert psnr(out[k], ref[k], peak=scale) >= PSNR_MIN, k
        assert_image_close(out["color"], ref["color"], 5e-4)
        gh = hip.backward(g["dL_dcolor"], g["dL_dinvdepth"], g["dL_dnormal"], g["dL_drefl"])
        names = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dnormals", "dL_drefl_strengths", "dL_dscales", "dL_drotations")
    for k in names:
        err = rel_maxnorm(gh[k].reshape(gr[k].shape), gr[k])
        assert err <= GRAD_TOL, (k, err)
        assert grad_gate(gh[k], gr[k], GRAD_TOL) <= GATE_BUDGET, (k, "elementwise gate")
    return out


def _hip(variant):
    return HipSurfel(_scene(variant)[0]) if variant == "S" else HipGauss(_scene(variant)[0], antialiasing=True)


# ------------------------------------------------------------------------------------------------ through the C ABI
class _Alloc:
    """A gsr_alloc_fn the test owns: torch allocates, the request for buffer `refuse` is answered with NULL."""

    def __init__(self, refuse=None):
        import _gsr
        self.bufs, self.requests, self.refuse = {}, [], refuse

        def cb(user, which, nbytes):
            self.requests.append((which, int(nbytes)))
            if which == self.refuse:
                return 0
            self.bufs[which] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
            return self.bufs[which].data_ptr()
        self.cb = _gsr.ALLOC_FN(cb)


ENTRIES = ("refl-plain", "refl-async-sort", "eval", "gauss", "eval-empty")


def _cabi_call(entry, alloc):
    """One call of the entry on the current stream.  Returns (rc, message, {output name: tensor}, everything that must stay alive until
    the stream has been synchronised)."""
    import _gsr
    lib, p = _gsr.lib, _gsr.ptr
    variant = "G" if entry == "gauss" else "S"
    kw, t, _ = _scene(variant)
    f = dict(dtype=torch.float32, device="cuda")
    n = 0 if entry == "eval-empty" else P
    radii = torch.empty(n, dtype=torch.int32, device="cuda")
    out = dict(color=torch.empty(3, H, W, **f), refl_map=torch.empty(H, W, **f), radii=radii)
    stream = torch.cuda.current_stream().cuda_stream
    common = (n, 3, 16, p(t["bg"]), W, H, p(t["means3D"]))
    camera = (p(t["viewmatrix"]), p(t["projmatrix"]), p(t["campos"]), float(kw["tanfovx"]), float(kw["tanfovy"]), 0)
    desc, keep = None, [t]
    if entry in ("refl-plain", "refl-async-sort", "eval-empty"):
        tex, fail, cam, _ = _reflection()
        out.update(final=torch.empty(3, H, W, **f), refl_color=torch.empty(3, H, W, **f), normal_world=torch.empty(3, H, W, **f),
                   rgba=torch.empty(6 * L * L * 4, **f))
        keys = scratch = None
        if entry == "refl-async-sort":
            keys = out["sort_keys"] = torch.empty(H * W, dtype=torch.int32, device="cuda")
            scratch = torch.empty(int(lib.gsr_deferred_reflection_scratch_floats(L, W, H, 1)), **f)
            keep.append(scratch)
        desc = _gsr.ReflForward(p(cam), p(tex), p(fail), L, p(out["rgba"]), p(out["final"]), p(out["refl_color"]), p(out["normal_world"]), p(keys),
                                p(scratch), scratch.numel() if scratch is not None else 0, 1 if scratch is not None else 0)
        keep.append(desc)
    if entry in ("refl-plain", "refl-async-sort"):
        out.update(others=torch.empty(8, H, W, **f), weights=torch.empty(P, **f))
        rc = lib.gsr_surfel_forward_refl(alloc.cb, None, *common, p(t["env_scope_mask"]), p(t["shs"]), None, p(t["refl_strengths"]), p(t["opacities"]),
                                         p(t["scales"]), 1.0, p(t["rotations"]), None, *camera, p(out["color"]), p(out["others"]), p(out["refl_map"]),
                                         p(radii), p(out["weights"]), ctypes.byref(desc), 0, stream)
    elif entry in ("eval", "eval-empty"):
        out["alpha"] = torch.empty(H, W, **f)
        if entry == "eval":
            out["normal_view"] = torch.empty(3, H, W, **f)
        rc = lib.gsr_surfel_forward_eval(alloc.cb, None, *common, p(t["shs"]), None, p(t["refl_strengths"]), p(t["opacities"]), p(t["scales"]), 1.0,
                                         p(t["rotations"]), None, *camera, p(out["color"]), p(out["alpha"]), p(out.get("normal_view")), p(out["refl_map"]),
                                         p(radii) if n else None, ctypes.byref(desc) if desc is not None else None, 0, stream)
    else:
        out.update(normal_map=torch.empty(3, H, W, **f), invdepth=torch.empty(H, W, **f))
        rc = lib.gsr_gauss_forward(alloc.cb, None, *common, p(t["shs"]), None, p(t["normals"]), p(t["refl_strengths"]), p(t["opacities"]), p(t["scales"]),
                                   1.0, p(t["rotations"]), None, *camera, p(out["color"]), p(out["normal_map"]), p(out["refl_map"]), p(out["invdepth"]), 1,
                                   p(radii), 0, stream)
    msg = lib.gsr_last_error().decode() if rc < 0 else ""
    return rc, msg, out, keep


def _settle():
    """What a caller does before it lets go of buffers the library may still use: join the side stream, wait for the device."""
    import _gsr
    assert _gsr.lib.gsr_side_join(torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _cabi_before(entry):
    """The well-formed call made BEFORE any refusal of this entry: (num_rendered, outputs on the host)."""
    alloc = _Alloc()
    rc, msg, out, keep = _cabi_call(entry, alloc)
    assert rc >= 0, msg
    _settle()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _fused_async_step():
    """One fused forward + backward of render() with a reflection gradient sink and an asynchronous tail: the cubemap / fail-value gradients
    (from the sink, behind side_join) and the parameter gradients."""
    import _gsr
    import gaussian_renderer as GR
    tex, fail, _, view = _reflection()
    names = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")
    t = {k: _scene("S")[1][k].clone().requires_grad_(True) for k in names}
    cm, fv = tex.clone().requires_grad_(True), fail.clone().requires_grad_(True)

    class Env:
        params = {"Cubemap_texture": cm, "Cubemap_failv": fv}

    class Pipe(_Pipe):
        gsr_reflection_grad_sink = {"cubemap": torch.zeros_like(tex), "fail": torch.zeros_like(fail)}
        gsr_async_reflection_tail = True
    pkg = GR.render(view, _model(t, Env, 3), Pipe, torch.tensor(BG, device="cuda"))
    weights = torch.from_numpy(S.make_upstream_grads(H, W, SEED)["dL_dcolor"]).cuda()
    (pkg["render"] * weights).sum().backward()
    _gsr.side_join()
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu().numpy() for k, v in t.items()}
    grads.update({k: v.cpu().numpy() for k, v in Pipe.gsr_reflection_grad_sink.items()})
    return grads


@pytest.mark.parametrize("entry, which", [(e, w) for e in ENTRIES[:4] for w in (GEOM, IMAGE, BINNING)] + [("eval-empty", IMAGE)],
                         ids=lambda v: v if isinstance(v, str) else {GEOM: "GEOM", IMAGE: "IMAGE", BINNING: "BINNING"}[v])
def test_cabi_refused_allocation_fails_cleanly(entry, which):
    import _gsr
    variant = "G" if entry == "gauss" else "S"
    R0, before = _cabi_before(entry)
    fused_before = _fused_async_step() if entry == "refl-async-sort" else None

    # ---- the refusal
    alloc = _Alloc(refuse=which)
    rc, msg, out, keep = _cabi_call(entry, alloc)
    assert rc == GSR_E_ALLOC, (rc, msg)
    refused = [nbytes for w, nbytes in alloc.requests if w == which]
    assert len(refused) == 1 and str(refused[0]) in msg, (alloc.requests, msg)
    torch.cuda.synchronize()      # the kernels already enqueued finish on the caller's buffers; no sticky error is left
    assert _gsr.lib.gsr_side_join(torch.cuda.current_stream().cuda_stream) == 0
    del out, keep, alloc

    # ---- the same thread, on the same stream, makes the well-formed call
    alloc = _Alloc()
    rc, msg, out, keep = _cabi_call(entry, alloc)
    assert rc >= 0, msg
    _settle()
    assert rc == R0
    for k, v in out.items():
        np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), before[k].view(np.uint8), err_msg=f"{k} differs from the call before the refusal")
    if entry == "eval-empty":
        assert rc == 0 and not before["color"].any() and not before["alpha"].any()
        return
    ref, state, _, _ = _oracle(variant)
    assert rc == ref["num_rendered"]
    np.testing.assert_array_equal(before["radii"], ref["radii"])
    fetch = lambda name, shape: _gsr.debug_fetch(0 if variant == "S" else 1, name, P, rc, W, H, alloc.bufs[GEOM], alloc.bufs[BINNING], alloc.bufs[IMAGE],
                                                 torch.int32, shape).cpu().numpy().astype(np.uint32)
    np.testing.assert_array_equal(fetch("point_list", (rc,)), state["point_list"])
    np.testing.assert_array_equal(fetch("ranges", (((W + 15) // 16) * ((H + 15) // 16), 2)), state["ranges"])
    colour_tol = 3e-5 if variant == "S" else 5e-4
    assert psnr(before["color"], ref["color"]) >= PSNR_MIN
    assert_image_close(before["color"], ref["color"], colour_tol)
    assert psnr(before["refl_map"], np.asarray(ref["refl_strength_map"]).reshape(H, W)) >= PSNR_MIN
    if entry == "eval":
        planes = [("alpha", ref["allmap"][1]), ("normal_view", ref["allmap"][2:5])]
    elif entry == "gauss":
        planes = [("normal_map", ref["normal_map"]), ("invdepth", ref["invdepth"])]
    else:
        planes = [("others", ref["allmap"])]
    for k, r in planes:
        a, r = before[k].reshape(-1, H, W), np.asarray(r).reshape(-1, H, W)
        for plane in range(r.shape[0]):
            assert psnr(a[plane], r[plane], peak=max(1.0, float(np.abs(r[plane]).max()))) >= PSNR_MIN, (k, plane)
    # images AND gradients of the next training call, as tests/test_gpu_parity.py holds them
    _check_rasterizer_against_oracle(variant, _hip(variant))
    if fused_before is not None:
        after = _fused_async_step()
        for k, b in fused_before.items():
            assert rel_maxnorm(after[k], b) <= 1e-5, k


# ------------------------------------------------------------------------------------------------ through Python
class _FailingTorch:
    """Stands in for the `torch` that _gsr.py sees: the n-th workspace request of _gsr.Workspace (a uint8 torch.empty of a positive size;
    its constructor's three are empty) raises `error`, everything else is torch's own."""

    def __init__(self, nth, error):
        self.nth, self.error, self.requests = nth, error, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        if kwargs.get("dtype") is torch.uint8 and args and isinstance(args[0], int) and args[0] > 0:
            self.requests += 1
            if self.requests == self.nth:
                raise self.error
        return torch.empty(*args, **kwargs)


def _render_model():
    tex, fail, _, view = _reflection()
    names = ("means3D", "shs", "opacities", "scales", "rotations", "refl_strengths")
    t = {k: _scene("S")[1][k].clone().requires_grad_(True) for k in names}

    class Env:
        params = {"Cubemap_texture": tex.clone().requires_grad_(True), "Cubemap_failv": fail.clone().requires_grad_(True)}
    return view, _model(t, Env, 3), t, Env


def _rasterizer(view):
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    kw, t, _ = _scene("S")
    return GaussianRasterizer(GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"], bg=t["bg"],
                                                            scale_modifier=1.0, viewmatrix=t["viewmatrix"], projmatrix=t["projmatrix"], sh_degree=3,
                                                            campos=t["campos"], prefiltered=False, debug=False))


def _drive(driver):
    """One forward of the driver: {name: tensor} of its outputs (and "_hip": the helper object of the two rasterizer drivers)."""
    import gaussian_renderer as GR
    if driver in ("rasterizer-S", "rasterizer-G"):
        hip = _hip(driver[-1])
        tensors = dict(color=hip.color, radii=hip.radii, refl_map=hip.refl_map)
        tensors.update(dict(allmap=hip.allmap, weights=hip.gw) if driver[-1] == "S" else dict(invdepth=hip.invdepth, normal_map=hip.normal_map))
        return dict(tensors, _hip=hip)
    view, pc, t, env = _render_model()
    bg = torch.tensor(BG, device="cuda")
    if driver == "rasterize_reflect":
        names = ("final", "refl_color", "rend_normal", "base_color", "radii", "allmap", "refl_map", "weights")
        ret = GR.rasterize_reflect(_rasterizer(view), env, view.world_view_transform, view.HWK, view.R, view.T, means3D=t["means3D"],
                                   means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"], shs=t["shs"], refl_strengths=t["refl_strengths"],
                                   scales=t["scales"], rotations=t["rotations"], env_scope_mask=_scene("S")[1]["env_scope_mask"])
        return dict(zip(names, ret))
    if driver == "rasterize_eval":
        with torch.no_grad():
            return GR.rasterize_eval(_rasterizer(view), t["means3D"], t["opacities"], shs=t["shs"], refl_strengths=t["refl_strengths"], scales=t["scales"],
                                     rotations=t["rotations"], env_map=env, world_view_transform=view.world_view_transform, HWK=view.HWK, R=view.R, T=view.T)
    if driver == "render":
        return {k: v for k, v in GR.render(view, pc, _Pipe, bg).items() if k != "viewspace_points"}
    assert driver == "render_fast"
    with torch.no_grad():
        return GR.render_fast(view, pc, _Pipe, bg)


DRIVERS = ("rasterizer-S", "rasterizer-G", "rasterize_reflect", "rasterize_eval", "render", "render_fast")


def _bits(out):
    return {k: v.detach().cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}


@functools.lru_cache(maxsize=None)
def _python_before(driver):
    with ctypes_binding():
        out = _bits(_drive(driver))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("nth", [1, 2, 3], ids=["first", "second", "third"])
@pytest.mark.parametrize("driver", DRIVERS)
def test_python_allocator_exception_reaches_the_caller(monkeypatch, driver, nth):
    import _gsr
    before = _python_before(driver)
    held = {dev: len(v) for dev, v in _gsr._side_held.items()}
    injected = OOM("injected: request %d of the workspace" % nth)
    with ctypes_binding():
        fake = _FailingTorch(nth, injected)
        monkeypatch.setattr(_gsr, "torch", fake)
        with pytest.raises(OOM) as caught:
            _drive(driver)
        monkeypatch.undo()
        assert caught.value is injected, "the caller got another exception than the one the allocation raised"
        assert fake.requests >= nth       # (the geometry and image requests come as a pair: the library makes the second after a refused first)
        # the library's own account of the failure may hang on it as context
        assert caught.value.__cause__ is None or isinstance(caught.value.__cause__, _gsr.GsrError)
        assert {dev: len(v) for dev, v in _gsr._side_held.items()} == held, "the failed call left tensors in _gsr._side_held"
        torch.cuda.synchronize()
        _gsr.side_join()
        assert not _gsr._side_held.get(torch.cuda.current_device())
        # ---- the next call of the same thread
        out = _drive(driver)
        after = _bits(out)
        assert set(after) == set(before)
        for k in before:
            np.testing.assert_array_equal(after[k].view(np.uint8), before[k].view(np.uint8), err_msg=f"{driver}: {k} differs from the run before the refusal")
        ref = _oracle("G" if driver == "rasterizer-G" else "S")[0]
        if "radii" in after:
            np.testing.assert_array_equal(after["radii"], ref["radii"])
        if "_hip" in out:
            _check_rasterizer_against_oracle(driver[-1], out["_hip"])
    _gsr.side_join()
    torch.cuda.synchronize()
