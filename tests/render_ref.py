"""Checker of the drop-in entry points (test infrastructure only; nothing under gaussian-splatting-reflection_amd/ imports this, and this
file imports nothing that needs a GPU).

The reference's render() (gaussian_renderer/__init__.py:42-219) restated from the pieces the suite already pins:

  rasterizer      oracle.SurfelOracle (scale_modifier, colors_precomp, cov3D_precomp and env_scope_mask are its own arguments)
  pixel passes    helpers_chain.surface_chain / shading_normal_chain / reference_chain in float64 with the oracle's cubemap
  host side       get_covariance_ref   scene/gaussian_model.py:34-40 with build_scaling_rotation / build_rotation of
                                       utils/general_utils.py:78-110 (the quaternion enters RAW: the reference passes self._rotation,
                                       so the normalisation inside build_rotation carries gradient)
                  transmats_ref        gaussian_renderer/__init__.py:97-106 (pipe.compute_cov3D_python)
                  env_scope_mask_ref   gaussian_renderer/__init__.py:79-85, strict `<` (train.py:63 uses `>` for the OUTSIDE mask of
                                       another loss term)
  loss            one scalar that reaches every differentiable output of the dictionary at once, with train.py:182-189 in it

The rasterizer is not differentiable torch: render_ref() returns the float64 chains built on LEAVES that hold the oracle's planes, so that
loss(...).backward() leaves the pixel gradients on those leaves (`pkg.leaves`) and `pkg.oracle.backward(...)` takes them from there.
"""
import numpy as np
import torch

from helpers_chain import reference_chain, shading_normal_chain, surface_chain

# reference lines 183-195 and 202-217, literally
KEYS_INITIAL = {"render", "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "rend_dist", "surf_depth",
                "surf_normal", "gaussian_weights", "env_scope_mask"}
KEYS_FULL = {"render", "viewspace_points", "visibility_filter", "radii", "rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal",
             "env_scope_mask", "refl_strength_map", "refl_color_map", "base_color_map", "gaussian_weights"}
LOSS_KEYS = ("render", "rend_alpha", "rend_normal", "rend_dist", "surf_depth", "surf_normal", "refl_strength_map", "refl_color_map",
             "base_color_map")
# every map but two is O(1).  surf_depth is a distance along the ray: the scenes of gsr_synth.make_scene lie 3 to 7 units deep, and the ray-splat
# intersection of an edge-on splat just behind the near plane reaches ~1e2.  rend_dist sums squared depth differences over pairs of blend weights:
# <= 7e-3 on those scenes.  Powers of two bring both per-tensor maxima to O(1), so that no term of the loss hides the others
WEIGHT_SCALE = {"surf_depth": 1.0 / 128.0, "rend_dist": 128.0}


# --------------------------------------------------------------------------------------------- the reference's host side
def build_rotation_ref(r):
    """utils/general_utils.py:78-99: (P,4) raw quaternions (w, x, y, z) -> (P,3,3), normalised inside."""
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def get_covariance_ref(xyz, scales, rotations, modifier=1.0):
    """GaussianModel.get_covariance(modifier) of the surfel model (scene/gaussian_model.py:34-40): the (P,4,4) splat-to-world matrix in
    row-vector form, rows 0-1 the tangent axes times (scale * modifier), row 2 the normal, row 3 the centre.  Differentiable torch in
    the dtype of its arguments."""
    s = torch.cat([scales * modifier, torch.ones_like(scales)], dim=-1)
    L = build_rotation_ref(rotations) * s[:, None, :3]                # R @ diag(s0, s1, 1)  (build_scaling_rotation, :101-110)
    RS = L.permute(0, 2, 1)
    P = xyz.shape[0]
    top = torch.cat([RS, torch.zeros((P, 3, 1), dtype=xyz.dtype, device=xyz.device)], dim=2)
    bottom = torch.cat([xyz, torch.ones((P, 1), dtype=xyz.dtype, device=xyz.device)], dim=1)[:, None, :]
    return torch.cat([top, bottom], dim=1)


def transmats_ref(cov, view):
    """gaussian_renderer/__init__.py:97-106: cov3D_precomp (P,9), column-major, from get_covariance_ref's matrices.  `view`: a camera
    dictionary of gsr_synth (W, H, znear, zfar, projmatrix = full_proj_transform)."""
    W, H, near, far = view["W"], view["H"], view["znear"], view["zfar"]
    ndc2pix = torch.tensor([[W / 2, 0, 0, (W - 1) / 2],
                            [0, H / 2, 0, (H - 1) / 2],
                            [0, 0, far - near, near],
                            [0, 0, 0, 1]], dtype=cov.dtype, device=cov.device).T
    world2pix = torch.as_tensor(view["projmatrix"]).to(dtype=cov.dtype, device=cov.device) @ ndc2pix
    return (cov[:, [0, 1, 3]] @ world2pix[:, [0, 1, 3]]).permute(0, 2, 1).reshape(-1, 9)


def env_scope_mask_ref(xyz, centre, radius):
    """gaussian_renderer/__init__.py:79-85: (P,) bool inside the sphere, strictly; a radius of 0 or less is the reference's (P,3)
    all-true tensor of which the rasterizer reads entry [id], i.e. all true."""
    xyz = np.asarray(xyz)
    if not radius > 0.0:
        return np.ones(xyz.shape[0], dtype=bool)
    c = np.asarray([float(v) for v in centre], dtype=xyz.dtype)
    return ((xyz - c[None]) ** 2).sum(axis=-1) < xyz.dtype.type(float(radius) ** 2)


# --------------------------------------------------------------------------------------------- render()
class Package(dict):
    """The reference's dictionary, with the checker's handles beside it: `oracle` (the SurfelOracle that holds the forward's state),
    `raster` (its forward's output), `leaves` (base, allmap, refl_map, cubemap, fail: float64 leaves the chains were built on)."""
    oracle = raster = leaves = None


def pixel_passes_ref(base, allmap, refl_map, tex, fail, cam, depth_ratio, initial_stage):
    """Reference lines 143-217 behind the rasterizer, float64 on the CPU, on the given planes (numpy).  Returns (maps, leaves)."""
    leaf = lambda x: torch.from_numpy(np.ascontiguousarray(x)).double().clone().requires_grad_(True)
    lv = dict(base=leaf(base), allmap=leaf(allmap), refl_map=leaf(refl_map), cubemap=leaf(tex), fail=leaf(fail))
    a = lv["allmap"]
    H, W = a.shape[1:]
    wvt, fpt = torch.from_numpy(cam["viewmatrix"]).double(), torch.from_numpy(cam["projmatrix"]).double()
    surf_depth, surf_normal = surface_chain(a, wvt, fpt, float(depth_ratio))
    out = {"rend_alpha": a[1:2], "rend_dist": a[6:7], "surf_depth": surf_depth, "surf_normal": surf_normal, "env_scope_mask": a[7:8]}
    if initial_stage:
        out["rend_normal"] = shading_normal_chain(a[2:5], wvt).permute(2, 0, 1)
        out["render"] = lv["base"]
    else:
        final, col, rn = reference_chain(a[2:5], lv["base"], lv["refl_map"], lv["cubemap"], lv["fail"], cam, W, H)
        out.update({"rend_normal": rn, "render": final, "refl_strength_map": lv["refl_map"], "refl_color_map": col, "base_color_map": lv["base"]})
    return out, lv


def raster_args(cam, scene, bg, sh_degree=3, scaling_modifier=1.0, override_color=None, env_scope_center=(0.0, 0.0, 0.0), env_scope_radius=0.0,
                compute_cov3D_python=False, dtype=np.float64):
    """The keyword arguments render() hands the rasterizer, for oracle.SurfelOracle.forward.  `scene`: numpy arrays means3D, shs, opacities,
    scales, rotations (raw), refl_strengths.  The host-side work (sphere test, homographies) is done in `dtype`."""
    f = lambda x: np.ascontiguousarray(np.asarray(x), dtype=dtype)
    kw = dict(bg=f(bg), means3D=scene["means3D"], opacities=scene["opacities"], viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"],
              campos=cam["campos"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=cam["H"], image_width=cam["W"],
              sh_degree=sh_degree, refl_strengths=scene["refl_strengths"], scale_modifier=float(scaling_modifier),
              env_scope_mask=env_scope_mask_ref(f(scene["means3D"]), env_scope_center, env_scope_radius))
    if override_color is None:
        kw["shs"] = scene["shs"]
    else:
        kw["colors_precomp"] = override_color
    if compute_cov3D_python:
        t = lambda k: torch.from_numpy(f(scene[k]))
        kw["cov3D_precomp"] = transmats_ref(get_covariance_ref(t("means3D"), t("scales"), t("rotations"), scaling_modifier), cam).numpy()
    else:
        kw["scales"], kw["rotations"] = scene["scales"], scene["rotations"]
    return kw


def render_ref(cam, scene, tex, fail, bg, sh_degree=3, scaling_modifier=1.0, override_color=None, initial_stage=False,
               env_scope_center=(0.0, 0.0, 0.0), env_scope_radius=0.0, depth_ratio=0.0, compute_cov3D_python=False, dtype=np.float64):
    """The reference's render() on the CPU: the oracle in `dtype`, the pixel passes in float64.  Returns a Package."""
    from oracle import oracle as orc
    o = orc.SurfelOracle(dtype)
    fo = o.forward(**raster_args(cam, scene, bg, sh_degree, scaling_modifier, override_color, env_scope_center, env_scope_radius,
                                 compute_cov3D_python, dtype))
    maps, leaves = pixel_passes_ref(fo["color"], fo["allmap"], fo["refl_strength_map"], tex, fail, cam, depth_ratio, initial_stage)
    pkg = Package(maps)
    pkg.update({"viewspace_points": torch.zeros(scene["means3D"].shape, dtype=torch.float64), "visibility_filter": torch.from_numpy(fo["radii"] > 0),
                "radii": torch.from_numpy(fo["radii"]), "gaussian_weights": torch.from_numpy(fo["gaussian_weights"])})
    pkg.oracle, pkg.raster, pkg.leaves = o, fo, leaves
    return pkg


# --------------------------------------------------------------------------------------------- the loss
def make_weights(H, W, seed):
    """Seeded N(0,1)/(H W) weights for every differentiable map of the dictionary (float64 numpy), scaled by WEIGHT_SCALE."""
    rs = np.random.RandomState(seed)
    planes = {k: 3 for k in ("render", "rend_normal", "surf_normal", "refl_color_map", "base_color_map")}
    return {k: rs.standard_normal((planes.get(k, 1), H, W)) / (H * W) * WEIGHT_SCALE.get(k, 1.0) for k in LOSS_KEYS}


def loss(pkg, weights):
    """sum_k <w_k, pkg[k]> over the keys of LOSS_KEYS the stage returns, plus the normal-consistency term of train.py:182-189 with
    opt.use_env_scope: mean((1 - (rend_normal * surf_normal).sum(0)) * env_scope_mask).  Works on either side: the weights are cast to the
    dtype and device of the maps."""
    total = 0.0
    for k in LOSS_KEYS:
        if k in pkg:
            total = total + (pkg[k] * torch.as_tensor(weights[k]).to(dtype=pkg[k].dtype, device=pkg[k].device)).sum()
    normal_error = (1 - (pkg["rend_normal"] * pkg["surf_normal"]).sum(dim=0))[None]
    return total + (normal_error * pkg["env_scope_mask"]).mean()


def backward_ref(maps, leaves, weights):
    """loss(maps, weights).backward() on the chains' leaves; returns {leaf name: float64 numpy gradient}, zeros for a leaf the stage does
    not read."""
    for t in leaves.values():
        t.grad = None
    loss(maps, weights).backward()
    return {k: (np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy().copy()) for k, t in leaves.items()}


def python_path_gradients(scene, cam, scaling_modifier, dL_dtransMat, dL_dmeans3D):
    """Gradient at (means3D, scales, raw rotations) of a render with pipe.compute_cov3D_python: the rasterizer's dL_dtransMat pulled back
    through float64 autograd of transmats_ref o get_covariance_ref, plus the rasterizer's direct dL_dmeans3D (the SH view direction)."""
    leaf = lambda k: torch.from_numpy(np.asarray(scene[k], dtype=np.float64)).clone().requires_grad_(True)
    x, s, r = leaf("means3D"), leaf("scales"), leaf("rotations")
    T = transmats_ref(get_covariance_ref(x, s, r, scaling_modifier), cam)
    T.backward(torch.from_numpy(np.asarray(dL_dtransMat, dtype=np.float64)).reshape(T.shape))
    return {"means3D": x.grad.numpy() + np.asarray(dL_dmeans3D, dtype=np.float64), "scales": s.grad.numpy(), "rotations": r.grad.numpy()}
