"""The entries of the Python surface as functions of a dictionary of named tensors, with one harness that calls an entry, runs one backward
with fixed upstream gradients and collects outputs and leaf gradients.  tests/test_gpu_layouts.py calls every entry with layout variants
(tests/layouts.py) and other dtypes of its tensors; tests/test_gpu_autograd_contract.py drives the autograd nodes behind the same entries.

An Entry knows
    base()     name -> contiguous float32 (or bool / int) device tensor, built once and never modified; other values pass through
    call(t)    runs the entry on t (same names; the harness has made leaves of the names in `diff`) and returns name -> output
    diff       the inputs that receive a gradient
    atomic     those of `diff` whose gradient is a sum formed by float atomics: per-Gaussian gradients of the two tile backwards (every
               pixel of a tile adds to its Gaussians), the cubemap / fail-value gradient of the reflection backward (rim pixels add to the
               staging texels directly and the run combine adds a workgroup's texel range in LDS, csrc/gsr_cubemap.hip) and of the cubemap
               encoder (one atomic per bilinear corner).  They are compared with the project's bound for "same arithmetic, atomics in
               another order" (ATOMIC_BOUND, as test_sort_drivers_agree_bit_for_bit); everything else bit for bit.
    vary       the tensor arguments a layout or dtype case replaces (default: every tensor of base())
    constant   name -> value: inputs that may be one value repeated (the `expanded` layout)
"""
import functools
import zlib

import numpy as np
import torch

from helpers import S, rel_maxnorm

ATOMIC_BOUND = 1e-5          # rel_maxnorm between two runs of the same arithmetic whose float atomics arrive in another order
LINEARITY_BOUND = 1e-4       # as test_c3_cull_bit_identity_and_backward_linearity: sums of two backwards against one backward of the sum

CONFIGS = {"a": dict(P=2003, W=200, H=120, deg=2, seed=61, mu=-2.8),       # M = 9: rows of 108 bytes, P * M * 3 * 4 is no multiple of 16
           "b": dict(P=6000, W=301, H=203, deg=3, seed=62, mu=-3.0)}       # ragged tile edges on both axes, M = 16
L = 16


class Env:
    def __init__(self, tex, fail):
        self.params = {"Cubemap_texture": tex, "Cubemap_failv": fail}


@functools.lru_cache(maxsize=None)
def scene(cfg):
    """Contiguous float32 device tensors of one small scene (never modified) and the camera's host values."""
    c = CONFIGS[cfg]
    P, W, H = c["P"], c["W"], c["H"]
    sc = S.make_scene(P, "S", seed=c["seed"], mu=c["mu"], mask_radius=6.0)
    cam = S.look_at_camera(W, H, eye=(0.3, -0.2, -0.8), target=(0, 0, 5))
    tex, fail = S.make_cubemap(L, 3, c["seed"])
    rs = np.random.RandomState(c["seed"])
    M = (c["deg"] + 1) ** 2
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {k: dev(sc[k]) for k in ("means3D", "opacities", "scales", "rotations", "refl_strengths")}
    t["shs"] = dev(sc["shs"][:, :M])
    t["mask"] = dev(sc["env_scope_mask"])
    assert 0 < int(t["mask"].sum()) < P
    t["colors"] = dev(rs.rand(P, 3).astype(np.float32))
    t["normals"] = dev(sc["normals"])
    t["scales3"] = dev(np.concatenate([sc["scales"], sc["scales"][:, :1] * 0.7], axis=1))
    t["cubemap"], t["fail"] = dev(tex), dev(fail + np.float32(0.25))
    t["bg"] = dev(np.array([0.1, 0.2, 0.3], np.float32))
    for k in ("viewmatrix", "projmatrix", "campos", "R", "T"):
        t[k] = dev(cam[k])
    info = dict(c, M=M, cam=cam, HWK=(H, W, cam["K"]), sc=sc)
    return t, info


@functools.lru_cache(maxsize=None)
def precomputed(cfg):
    """transMat (P,9) and cov3D (P,6) of the scene, from the CPU oracle's forward (as tests/test_gpu_api_paths.py)."""
    from oracle import oracle as orc
    t, info = scene(cfg)
    cam, sc = info["cam"], info["sc"]
    kw = dict(bg=np.zeros(3, np.float32), means3D=sc["means3D"], opacities=sc["opacities"], viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"],
              campos=cam["campos"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=info["H"], image_width=info["W"],
              sh_degree=info["deg"], shs=sc["shs"][:, :info["M"]], refl_strengths=sc["refl_strengths"], rotations=sc["rotations"])
    o = orc.SurfelOracle(np.float32)
    o.forward(scales=sc["scales"], env_scope_mask=sc["env_scope_mask"], **kw)
    T = o.state("transMat")
    T[~(o.state("radii") > 0)] = np.eye(3, dtype=np.float32).reshape(-1)
    g = orc.GaussOracle(np.float32)
    g.forward(scales=t["scales3"].cpu().numpy(), normals=sc["normals"], **kw)
    cov = g.state("cov3D")
    cov[~(g.state("radii") > 0)] = np.array([1e-2, 0, 0, 1e-2, 0, 1e-2], np.float32)
    return torch.from_numpy(np.ascontiguousarray(T, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(cov, np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def maps(cfg):
    """The rasterizer's planes of the scene (no grad): inputs of the per-pixel passes and of the losses."""
    e = SURFEL[("shs", cfg)]
    with torch.no_grad():
        out = e.call(dict(e.base()))
    return {k: v.clone() for k, v in out.items()}


def upstream(name, shape, dtype=torch.float32):
    """The fixed upstream gradient of output `name`: N(0,1) / pixels, from a seed that depends on the name alone."""
    return _upstream(name, tuple(shape)).to(dtype)


@functools.lru_cache(maxsize=None)
def _upstream(name, shape):
    gen = torch.Generator(device="cpu").manual_seed(zlib.crc32(name.encode()))
    if len(shape) == 0:
        return torch.tensor(1.75, device="cuda")
    px = shape[-1] * shape[-2] if len(shape) >= 2 else shape[0]
    return (torch.randn(shape, generator=gen) / px).cuda()


class Entry:
    def __init__(self, name, base, call, diff=(), atomic=(), vary=None, constant=None, converts=(), zero_ok=("fail",)):
        self.name, self.base, self.call = name, base, call
        self.zero_ok = tuple(zero_ok)          # gradients that may be all zero in the reference call
        self.diff, self.atomic = tuple(diff), frozenset(atomic)
        self._vary, self.constant = vary, dict(constant or {})
        self.converts = tuple(converts)        # inputs the binding converts with .float() (other dtypes are accepted)

    @property
    def vary(self):
        if self._vary is not None:
            return tuple(self._vary)
        return tuple(k for k, v in self.base().items() if torch.is_tensor(v) and v.numel() > 0)


def run(entry, tensors, outputs=None, backward=True, frozen=()):
    """One call of `entry` on `tensors` and one backward through `sum(out * upstream(out))` over its differentiable outputs (`outputs`:
    only those names).  frozen: inputs of entry.diff that do not require grad in this call.  Returns (outputs detached, gradients by
    input name, the leaves)."""
    t = {}
    for k, v in tensors.items():
        if torch.is_tensor(v) and k in entry.diff and k not in frozen and v.is_floating_point():
            t[k] = v.detach().requires_grad_(True)
        else:
            t[k] = v
    out = entry.call(t)
    diff_out = {k: o for k, o in out.items() if torch.is_tensor(o) and o.requires_grad and (outputs is None or k in outputs)}
    if backward and diff_out:
        loss = None
        for k, o in diff_out.items():
            term = (o * upstream(k, o.shape)).sum()
            loss = term if loss is None else loss + term
        loss.backward()
    grads = {k: t[k].grad for k in entry.diff if torch.is_tensor(t.get(k)) and t[k].requires_grad}
    return {k: (o.detach() if torch.is_tensor(o) else o) for k, o in out.items()}, grads, t


def same_bits(a, b):
    """torch.equal, with NaNs allowed where both have one (the angular error map marks invalid pixels with NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        return bool(((a == b) | (a.isnan() & b.isnan())).all())
    return torch.equal(a, b)


def compare(entry, ref, got, what, leaves=None, check_nonzero=True):
    """`got` = (outputs, grads) against `ref`: outputs and deterministic gradients bit for bit, atomically reduced gradients to
    ATOMIC_BOUND.  leaves: the inputs of `got`; a gradient has its leaf's shape and dtype whatever its strides."""
    (ro, rg), (go, gg) = ref, got
    assert sorted(ro) == sorted(go), what
    for k, r in ro.items():
        if torch.is_tensor(r):
            assert same_bits(go[k], r), (entry.name, what, "output", k, float((go[k].double() - r.double()).abs().max()) if go[k].shape == r.shape else go[k].shape)
        else:
            assert go[k] == r, (entry.name, what, "output", k)
    assert sorted(rg) == sorted(gg), (entry.name, what, sorted(rg), sorted(gg))
    for k, r in rg.items():
        g = gg[k]
        assert (g is None) == (r is None), (entry.name, what, "gradient", k)
        if r is None:
            continue
        if leaves is not None:
            assert g.shape == leaves[k].shape and g.dtype == leaves[k].dtype, (entry.name, what, "gradient shape / dtype", k)
        assert g.shape == r.shape, (entry.name, what, k)
        if k in entry.atomic:
            err = rel_maxnorm(g.double().cpu().numpy(), r.double().cpu().numpy())
            assert err <= ATOMIC_BOUND, (entry.name, what, "gradient", k, err)
        else:
            # (a leaf of another dtype receives the float32 gradient cast to its own)
            assert same_bits(g, r.to(g.dtype)), (entry.name, what, "gradient", k, float((g.double() - r.double()).abs().max()))


def reference(entry, base=None):
    """(outputs, grads) of the entry on contiguous float32 clones, and the same once more: the second must satisfy compare() against the
    first, which shows that the bounds are reachable by the reference alone (and that what is compared bit for bit is deterministic)."""
    base = entry.base() if base is None else base
    clones = lambda: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    o1, g1, _ = run(entry, clones())
    o2, g2, _ = run(entry, clones())
    compare(entry, (o1, g1), (o2, g2), "reference repeated")
    for k, g in g1.items():
        # (no pixel of these views has a zero reflection vector, so only the encoder's own test reaches the fail value)
        assert g is not None and bool(torch.isfinite(g).all()) and (float(g.abs().max()) > 0 or k in entry.zero_ok), (entry.name, "a zero reference gradient compares nothing", k)
    return o1, g1


# ------------------------------------------------------------------------------------------------------------------ rasterizers
def _settings(mod, t, info, **extra):
    cam = info["cam"]
    return mod.GaussianRasterizationSettings(image_height=info["H"], image_width=info["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t["bg"],
                                             scale_modifier=1.0, viewmatrix=t["viewmatrix"], projmatrix=t["projmatrix"], sh_degree=info["deg"],
                                             campos=t["campos"], prefiltered=False, debug=False, **extra)


RASTER_PARAMS = ("means3D", "means2D", "opacities", "refl_strengths", "shs", "colors", "scales", "rotations", "transmat", "cov3D", "normals")
CAMERA = ("bg", "viewmatrix", "projmatrix", "campos")


def _surfel_entry(form, cfg, tap=False):
    """tap: also the output tap `normal_view` (allmap[2:5] as an output of its own, what render() hands the reflection pass)."""
    def base():
        t, info = scene(cfg)
        b = {k: t[k] for k in CAMERA + ("means3D", "opacities", "refl_strengths", "mask")}
        b["means2D"] = torch.zeros_like(t["means3D"])
        b.update({"colors": t["colors"]} if form == "colors" else {"shs": t["shs"]})
        b.update({"transmat": precomputed(cfg)[0]} if form == "transmat" else {"scales": t["scales"], "rotations": t["rotations"]})
        return b

    def call(t):
        import diff_surfel_rasterization as dsr
        rast = dsr.GaussianRasterizer(_settings(dsr, t, scene(cfg)[1]))
        if tap:
            rast.set_output_taps(("normal_view",))
        color, radii, allmap, refl_map, gw, *taps = rast(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t.get("shs"),
                                                  colors_precomp=t.get("colors"), refl_strengths=t["refl_strengths"], scales=t.get("scales"),
                                                  rotations=t.get("rotations"), cov3D_precomp=t.get("transmat"), env_scope_mask=t["mask"])
        out = dict(color=color, radii=radii, allmap=allmap, refl_map=refl_map, gw=gw)
        if tap:
            out["normal_view"] = taps[0]
        return out
    return Entry(f"surfel-{form}-{cfg}{'-tap' if tap else ''}", base, call, diff=RASTER_PARAMS, atomic=RASTER_PARAMS, constant={"opacities": 0.6, "refl_strengths": 0.2, "bg": 0.25})


def _gauss_entry(form, cfg, antialiasing):
    def base():
        t, info = scene(cfg)
        b = {k: t[k] for k in CAMERA + ("means3D", "opacities", "refl_strengths", "normals")}
        b["means2D"] = torch.zeros_like(t["means3D"])
        b.update({"colors": t["colors"], "cov3D": precomputed(cfg)[1]} if form == "cov3D" else {"shs": t["shs"], "scales": t["scales3"], "rotations": t["rotations"]})
        return b

    def call(t):
        import diff_gaussian_rasterization as dgr
        rast = dgr.GaussianRasterizer(_settings(dgr, t, scene(cfg)[1], antialiasing=antialiasing))
        color, radii, invdepth, normal_map, refl_map = rast(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t.get("shs"),
                                                            colors_precomp=t.get("colors") if form == "cov3D" else None, normals=t["normals"],
                                                            refl_strengths=t["refl_strengths"], scales=t.get("scales"), rotations=t.get("rotations"),
                                                            cov3D_precomp=t.get("cov3D"))
        return dict(color=color, radii=radii, invdepth=invdepth, normal_map=normal_map, refl_map=refl_map)
    return Entry(f"gauss-{form}-{cfg}-aa{int(antialiasing)}", base, call, diff=RASTER_PARAMS, atomic=RASTER_PARAMS,
                 constant={"opacities": 0.6, "refl_strengths": 0.2, "bg": 0.25})


SURFEL = {(form, cfg): _surfel_entry(form, cfg) for form, cfg in (("shs", "a"), ("shs", "b"), ("colors", "a"), ("transmat", "a"))}
GAUSS = {(form, cfg, aa): _gauss_entry(form, cfg, aa) for form, cfg, aa in (("shs", "a", False), ("shs", "b", True), ("cov3D", "a", True))}


def _mark_visible_entry(variant, cfg):
    def base():
        t, _ = scene(cfg)
        b = {k: t[k] for k in ("bg", "viewmatrix", "projmatrix", "campos")}
        b["means3D"] = t["means3D"].clone()
        b["means3D"][::3, 2] = -1.0 - b["means3D"][::3, 2]        # every third point behind the camera
        return b

    def call(t):
        import diff_gaussian_rasterization as dgr
        import diff_surfel_rasterization as dsr
        mod = dsr if variant == "S" else dgr
        extra = {} if variant == "S" else {"antialiasing": False}
        present = mod.GaussianRasterizer(_settings(mod, t, scene(cfg)[1], **extra)).markVisible(t["means3D"])
        assert 0 < int(present.sum()) < present.numel()
        return dict(present=present)
    return Entry(f"markVisible-{variant}-{cfg}", base, call, vary=("viewmatrix", "projmatrix", "means3D"))


MARK_VISIBLE = {v: _mark_visible_entry(v, "a") for v in ("S", "G")}


# ------------------------------------------------------------------------------------------------------------------ gaussian_renderer
REFL_INPUTS = ("cubemap", "fail", "R", "T")


def _fused_entry(cfg, frozen_env=False):
    """gaussian_renderer.rasterize_reflect.  t["_sinks"] (optional, not a tensor): (rasterizer sink | None, reflection sink | None, accumulate,
    async_tail) of this call."""

    def base():
        t, info = scene(cfg)
        b = {k: t[k] for k in CAMERA + ("means3D", "opacities", "refl_strengths", "mask", "shs", "scales", "rotations") + REFL_INPUTS}
        b["means2D"] = torch.zeros_like(t["means3D"])
        return b

    def call(t):
        import diff_surfel_rasterization as dsr
        from gaussian_renderer import rasterize_reflect
        info = scene(cfg)[1]
        rast = dsr.GaussianRasterizer(_settings(dsr, t, info))
        raster_sink, rs, accumulate, async_tail = t.get("_sinks", (None, None, False, False))
        rast.set_grad_sink(raster_sink, accumulate)
        final, refl_color, nworld, basec, radii, allmap, refl_map, gw = rasterize_reflect(
            rast, Env(t["cubemap"], t["fail"]), t["viewmatrix"], info["HWK"], t["R"], t["T"], means3D=t["means3D"], means2D=t["means2D"],
            opacities=t["opacities"], shs=t["shs"], refl_strengths=t["refl_strengths"], scales=t["scales"], rotations=t["rotations"],
            env_scope_mask=t["mask"], refl_grad_sink=rs, accumulate=accumulate and bool(rs), async_tail=async_tail and bool(rs))
        return dict(final=final, refl_color=refl_color, nworld=nworld, base=basec, radii=radii, allmap=allmap, refl_map=refl_map, gw=gw)
    diff = tuple(k for k in RASTER_PARAMS + ("cubemap", "fail") if not (frozen_env and k in ("cubemap", "fail")))
    return Entry(f"rasterize_reflect-{cfg}{'-frozen-env' if frozen_env else ''}", base, call, diff=diff, atomic=RASTER_PARAMS + ("cubemap", "fail"),
                 constant={"opacities": 0.6, "refl_strengths": 0.2, "bg": 0.25})


FUSED = {cfg: _fused_entry(cfg) for cfg in ("a", "b")}


def _pixel_base(cfg, names):
    t, info = scene(cfg)
    m = maps(cfg)
    b = {"normal_view": m["allmap"][2:5].clone(), "base_color": m["color"], "refl_map": m["refl_map"], "allmap": m["allmap"]}
    b.update({k: t[k] for k in ("cubemap", "fail", "viewmatrix", "projmatrix", "R", "T")})
    return {k: b[k] for k in names}


def _deferred_entry(cfg):
    names = ("normal_view", "base_color", "refl_map", "cubemap", "fail", "viewmatrix", "R", "T")

    def call(t):
        from gaussian_renderer import deferred_reflection
        final, refl_color, nworld = deferred_reflection(t["normal_view"], t["base_color"], t["refl_map"], Env(t["cubemap"], t["fail"]), t["viewmatrix"],
                                                        scene(cfg)[1]["HWK"], t["R"], t["T"])
        return dict(final=final, refl_color=refl_color, nworld=nworld)
    return Entry(f"deferred_reflection-{cfg}", lambda: _pixel_base(cfg, names), call, diff=names[:5], atomic=("cubemap", "fail"), converts=names[:5])


def _shading_entry(cfg):
    names = ("normal_view", "viewmatrix", "R", "T")

    def call(t):
        from gaussian_renderer import shading_normal
        return dict(nworld=shading_normal(t["normal_view"], t["viewmatrix"], scene(cfg)[1]["HWK"], t["R"], t["T"]))
    return Entry(f"shading_normal-{cfg}", lambda: _pixel_base(cfg, names), call, diff=names[:1], converts=names[:1])


class View:
    """A camera object as gaussian_renderer reads it."""

    def __init__(self, t, info):
        cam = info["cam"]
        self.FoVx, self.FoVy, self.image_width, self.image_height = cam["FoVx"], cam["FoVy"], info["W"], info["H"]
        self.world_view_transform, self.full_proj_transform, self.camera_center = t["viewmatrix"], t["projmatrix"], t.get("campos")
        self.HWK, self.R, self.T, self.znear, self.zfar = info["HWK"], t.get("R"), t.get("T"), cam["znear"], cam["zfar"]


def _surface_entry(cfg):
    names = ("allmap", "viewmatrix", "projmatrix")

    def call(t):
        from gaussian_renderer import surface_pass
        sd, sn = surface_pass(t["allmap"], View(t, scene(cfg)[1]), 0.3)
        return dict(surf_depth=sd, surf_normal=sn)
    return Entry(f"surface_pass-{cfg}", lambda: _pixel_base(cfg, names), call, diff=names[:1], converts=names[:1])


def _eval_entry(cfg, env):
    def base():
        t, info = scene(cfg)
        return {k: t[k] for k in CAMERA + ("means3D", "opacities", "refl_strengths", "shs", "scales", "rotations") + (REFL_INPUTS if env else ())}

    def call(t):
        import diff_surfel_rasterization as dsr
        from gaussian_renderer import rasterize_eval
        info = scene(cfg)[1]
        rast = dsr.GaussianRasterizer(_settings(dsr, t, info))
        kw = dict(env_map=Env(t["cubemap"], t["fail"]), world_view_transform=t["viewmatrix"], HWK=info["HWK"], R=t["R"], T=t["T"]) if env else {}
        with torch.no_grad():
            return rasterize_eval(rast, t["means3D"], t["opacities"], shs=t["shs"], refl_strengths=t["refl_strengths"], scales=t["scales"],
                                  rotations=t["rotations"], **kw)
    return Entry(f"rasterize_eval-{cfg}-env{int(env)}", base, call)


PIXEL = {"deferred_reflection": _deferred_entry("b"), "shading_normal": _shading_entry("b"), "surface_pass": _surface_entry("b")}
EVAL = {"eval-env": _eval_entry("a", True), "eval-plain": _eval_entry("a", False)}


def _render_entry(cfg, fast, initial_stage, no_grad=False):
    """render() / render_fast() on a camera object and a model whose tensors are the (laid out) inputs.  no_grad: render_fast's
    inference-only forward."""
    def base():
        t, info = scene(cfg)
        return {k: t[k] for k in CAMERA + ("means3D", "opacities", "refl_strengths", "shs", "scales", "rotations") + REFL_INPUTS}

    def call(t):
        import gaussian_renderer as gr
        info = scene(cfg)[1]

        class PC:
            get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (t["means3D"], t["opacities"], t["scales"], t["rotations"], t["shs"],
                                                                                       t["refl_strengths"])
            active_sh_degree, get_envmap = info["deg"], Env(t["cubemap"], t["fail"])

        class Pipe:
            depth_ratio, compute_cov3D_python = 0.0, False
        view = View(t, info)
        if no_grad:
            with torch.no_grad():
                pkg = gr.render_fast(view, PC, Pipe, t["bg"], initial_stage=initial_stage)
        elif fast:
            pkg = gr.render_fast(view, PC, Pipe, t["bg"], initial_stage=initial_stage)
        else:
            pkg = gr.render(view, PC, Pipe, t["bg"], initial_stage=initial_stage)
        return {k: v for k, v in pkg.items() if k != "viewspace_points"}
    diff = () if no_grad else ("means3D", "opacities", "refl_strengths", "shs", "scales", "rotations") + (() if initial_stage else ("cubemap", "fail"))
    # (the initial stage returns no reflection-strength plane: that parameter's gradient is all zero there)
    return Entry(f"render{'_fast' if fast else ''}-{cfg}-initial{int(initial_stage)}{'-no_grad' if no_grad else ''}", base, call, diff=diff, atomic=RASTER_PARAMS + ("cubemap", "fail"),
                 zero_ok=("fail", "refl_strengths") if initial_stage else ("fail",))


RENDER = {"render": _render_entry("a", False, False), "render-initial": _render_entry("a", False, True), "render_fast": _render_entry("a", True, False),
          "render_fast-no_grad": _render_entry("a", True, False, no_grad=True), "render_fast-no_grad-initial": _render_entry("a", True, True, no_grad=True)}


# ------------------------------------------------------------------------------------------------------------------ losses, encoder
def _images(cfg):
    m = maps(cfg)
    info = scene(cfg)[1]
    gen = torch.Generator(device="cpu").manual_seed(5)
    gt = torch.rand((3, info["H"], info["W"]), generator=gen).cuda()
    return (0.7 * gt + 0.3 * m["color"]).clamp(0, 1).contiguous(), gt


def _loss_entry(which, cfg):
    def base():
        img, gt = _images(cfg)
        return {"image": img, "gt": gt}

    def call(t):
        from utils import loss_utils as lu
        lu.clear_cache()
        if which == "l1":
            return dict(loss=lu.l1_loss(t["image"], t["gt"]))
        if which == "ssim":
            return dict(loss=lu.ssim(t["image"], t["gt"]))
        if which == "l1+ssim":          # the reference's loop: two calls on the same pair share one node
            return dict(l1=lu.l1_loss(t["image"], t["gt"]), ssim=lu.ssim(t["image"], t["gt"]))
        return dict(loss=lu.photometric_loss(t["image"], t["gt"], 0.2))
    return Entry(f"{which}-{cfg}", base, call, diff=("image",))


def _normal_loss_entry(cfg, masked):
    def base():
        m = maps(cfg)
        t, info = scene(cfg)
        gen = torch.Generator(device="cpu").manual_seed(6)
        n = torch.randn((3, info["H"], info["W"]), generator=gen).cuda()
        b = {"rend_normal": torch.nn.functional.normalize(m["allmap"][2:5] + 0.05 * n, dim=0).contiguous(),
             "surf_normal": torch.nn.functional.normalize(n, dim=0).contiguous()}
        if masked:
            b["mask"] = m["allmap"][7:8].clone()
        return b

    def call(t):
        from utils.loss_utils import normal_consistency_loss
        return dict(loss=normal_consistency_loss(t["rend_normal"], t["surf_normal"], 0.05, t.get("mask")))
    return Entry(f"normal_loss-{cfg}-mask{int(masked)}", base, call, diff=("rend_normal", "surf_normal"), converts=("rend_normal", "surf_normal", "mask"))


def _cubemap_entry():
    def base():
        t, _ = scene("a")
        gen = torch.Generator(device="cpu").manual_seed(8)
        d = torch.randn((4099, 3), generator=gen)
        d[::97] = 0.0           # zero directions take the fail value
        return {"dirs": d.cuda(), "cubemap": t["cubemap"], "fail": t["fail"]}

    def call(t):
        from cubemapencoder.cubemap_encoder import cubemap_encode
        return dict(features=cubemap_encode(t["dirs"], t["cubemap"], t["fail"], 1, 1))
    return Entry("cubemapencoder", base, call, diff=("dirs", "cubemap", "fail"), atomic=("cubemap", "fail"), converts=("dirs", "cubemap", "fail"), zero_ok=())


LOSSES = {w: _loss_entry(w, "b") for w in ("l1", "ssim", "l1+ssim", "photometric")}
LOSSES.update({"normal_loss": _normal_loss_entry("b", False), "normal_loss-masked": _normal_loss_entry("b", True), "cubemapencoder": _cubemap_entry()})


# ------------------------------------------------------------------------------------------------------------------ metrics, presentation
def _metrics_entry(cfg, quantize8):
    def base():
        img, gt = _images(cfg)
        m = maps(cfg)
        t, _ = scene(cfg)
        return {"image": (img * 1.2 - 0.1).contiguous(), "gt": gt, "alpha": m["allmap"][1:2].clone(), "gt_mask": (gt[0:1] > 0.3).float(), "bg": t["bg"]}

    def call(t):
        from gsr_eval import MetricsTable
        table = MetricsTable(2, t["image"].device)
        u8 = [torch.zeros(t["image"].shape, dtype=torch.uint8, device="cuda") for _ in range(2)] if quantize8 else [None, None]
        table.image(1, t["image"], t["gt"], clamp=True, alpha=t["alpha"], gt_mask=t["gt_mask"], background=t["bg"], quantize8=quantize8,
                    img_u8=u8[0], gt_u8=u8[1])
        out = dict(row=table.rows[1].clone())
        if quantize8:
            out.update(img_u8=u8[0], gt_u8=u8[1])
        return out
    return Entry(f"metrics-image-{cfg}-q{int(quantize8)}", base, call)


def _normal_mae_entry(cfg):
    def base():
        b = _normal_loss_entry(cfg, False).base()
        return {"pred": b["rend_normal"], "gt": b["surf_normal"]}

    def call(t):
        from gsr_eval import MetricsTable
        from utils.mae_utils import angular_error_map, compute_mae
        table = MetricsTable(1, t["pred"].device)
        table.normals(0, t["pred"], t["gt"])
        return dict(row=table.rows[0].clone(), error_map=angular_error_map(t["pred"], t["gt"]), mae=compute_mae(t["pred"][None], t["gt"][None]))
    return Entry(f"normal_mae-{cfg}", base, call)


def _present_entry(cfg):
    items = ["RGB", "Alpha", "Normal", "Depth", "Curvature", "Refl. Strength"]

    def base():
        m = maps(cfg)
        img, gt = _images(cfg)
        return {"render": img, "gt": gt, "rend_alpha": m["allmap"][1:2].clone(), "rend_normal": m["allmap"][2:5].clone(), "surf_depth": m["allmap"][0:1].clone(),
                "refl_strength_map": m["refl_map"]}

    def call(t):
        from utils import image_utils as iu
        out = dict(psnr=iu.psnr(t["render"], t["gt"]), mse=iu.mse(t["render"], t["gt"]), gradient_map=iu.gradient_map(t["render"]),
                   colormap=iu.colormap(t["surf_depth"]))
        for mode, name in enumerate(items):
            out[f"float-{name}"] = iu.render_net_image(t["render"], t, items, mode).clone()
            out[f"bytes-{name}"] = iu.present_bytes(t["render"], t, items, mode)
        return out
    return Entry(f"present-{cfg}", base, call, vary=("render", "gt", "rend_alpha", "rend_normal", "surf_depth", "refl_strength_map"))


METRICS = {"metrics-image-q8": _metrics_entry("b", True), "metrics-image": _metrics_entry("b", False), "normal_mae": _normal_mae_entry("b"),
           "present": _present_entry("b")}


# ------------------------------------------------------------------------------------------------------------------ densification, KNN
def _densify_stats_entry():
    def base():
        P = 2003
        rs = np.random.RandomState(1)
        return {"viewspace_grad": torch.from_numpy((rs.randn(P, 3) * 1e-3).astype(np.float32)).cuda(),
                "radii": torch.from_numpy((rs.rand(P) < 0.6).astype(np.int32) * rs.randint(1, 40, P).astype(np.int32)).cuda(),
                "gaussian_weights": torch.from_numpy((rs.rand(P) * (rs.rand(P) < 0.5)).astype(np.float32)).cuda()}

    def call(t):
        from gsr_densify import DensifyStats
        stats = DensifyStats(2003, "cuda")
        for _ in range(2):
            stats.update(t["viewspace_grad"], t["radii"], t["gaussian_weights"])
        return dict(buf=stats.buf)
    return Entry("DensifyStats.update", base, call)


def _knn_entry():
    def base():
        return {"points": scene("a")[0]["means3D"]}

    def call(t):
        from simple_knn._C import distCUDA2
        return dict(dist2=distCUDA2(t["points"]))
    return Entry("distCUDA2", base, call)


SMALL = {"DensifyStats.update": _densify_stats_entry(), "distCUDA2": _knn_entry()}
