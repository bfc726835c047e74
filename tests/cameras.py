"""Dataset-style cameras for the tests (test infrastructure only): anisotropic focal lengths, off-centre principal points, rolled
poses, narrow and wide fields of view, and image sizes at which the surfel backward's int(focal * tan * 2) comes out one short.

gsr_synth.make_camera (the benchmark's builder) always gives fx == fy, the principal point at the image centre and, in most tests, an
identity view matrix; with such a camera focal_x / focal_y, limx / limy, W/2 / H/2 and the entries of K can be swapped in a kernel
without any test seeing it.  The reference trains on COLMAP PINHOLE cameras, built through its (H, W, K) path; hwk_camera() builds
the same matrices from (W, H, fx, fy, cx, cy, R, T), pinned against tests/golden/camera_hwk_golden.npz.

  family(name, W, H, seed) -> camera dict, name in FAMILIES:
    aniso      fx / fy = 1.4 (even seed) or 1 / 1.4 (odd seed)
    offcentre  cx, cy 10-20 % of the size away from the centre, the two signs from the seed's low bits
    rolled     roll about 35 deg plus pitch and yaw, T != 0: no 3x3 block of the view matrix is symmetric
    narrow     FoVy 12 deg          wide   FoVy 110 deg
    trunc      (W, fx) and (H, fy) found by trunc_search(): the surfel backward rebuilds its homography for W - 1 and H - 1
               (the image size differs from the requested one by a few pixels: the search moves it)
    trunc_x    the sibling of trunc: same size, same fx, fy moved by a few ulps to the nearest value that does NOT truncate
    all        anisotropic, off-centre, rolled and truncating at once
  frustum_scene(variant, P, cam, seed) -> kw of helpers.scene_kwargs, Gaussians drawn in VIEW space over 1.6 x the frustum at depths
               0.15 .. 0.2 (in front of the near plane) and 1 .. 8, mapped to world space with the inverse view, so that every family
               sees visible, off-screen, near-culled and (variant G) frustum-clamped Gaussians wherever its camera looks.
"""
import math

import numpy as np

import adversarial_scenes as A
from adversarial_scenes import S

FAMILIES = ("aniso", "offcentre", "rolled", "narrow", "wide", "trunc", "all")
# the scenes tests/test_gpu_cameras.py renders and tests/test_cameras_host.py measures: P Gaussians, requested (ragged) size, base seed.
# Variant S takes the camera of the base seed and variant G that of base + 1, so that between them both focal ratios and different
# principal-point quadrants are rendered.
P_SCENE, W_SCENE, H_SCENE = 3000, 200, 136
NEAR_FRAC = 0.06        # share of a scene's Gaussians placed in front of the near plane (view depth 0.15 .. 0.2: culled)
SEEDS = {"aniso": 10, "offcentre": 20, "rolled": 30, "narrow": 40, "wide": 50, "trunc": 61, "trunc_x": 61, "all": 70}


def scene(name, variant, P=P_SCENE, W=W_SCENE, H=H_SCENE):
    """(kw, cam) of a family's scene for variant "S" or "G".  trunc and trunc_x share the scene seed: the same Gaussians in view space."""
    seed = SEEDS[name] + (variant == "G")
    cam = family(name, W, H, seed)
    return frustum_scene(variant, P, cam, 100 + seed), cam


def trunc_pair(variant="S"):
    """(kw, kw_x, cam): the trunc scene, and the SAME Gaussians under the sibling camera trunc_x (only tanfovy and the projection move,
    by a few ulps)."""
    kw, cam = scene("trunc", variant)
    cam_x = family("trunc_x", W_SCENE, H_SCENE, SEEDS["trunc_x"] + (variant == "G"))
    assert (cam_x["W"], cam_x["H"], cam_x["tanfovx"]) == (cam["W"], cam["H"], cam["tanfovx"])
    return kw, dict(kw, tanfovy=cam_x["tanfovy"], projmatrix=cam_x["projmatrix"]), cam


# ------------------------------------------------------------------------------------------- builder
def hwk_camera(W, H, fx, fy, cx, cy, R=None, T=None, znear=0.01, zfar=100.0):
    """Camera dictionary of gsr_synth.make_camera for a pinhole camera given by its intrinsics.  R is the camera-to-world rotation and T
    the world-to-camera translation, as the reference stores them.  The frustum is the one whose near-plane window is the image as seen
    through K: it reaches cx / fx to one side of the optical axis and (W - cx) / fx to the other, so the projection has the scale
    2 fx / W and the offset 2 cx / W - 1 in x (2 fy / H and 2 cy / H - 1 in y), entries rounded to float32 as the reference holds the
    matrix.  tanfovx = W / (2 fx) and tanfovy = H / (2 fy): the reference's dataset readers derive the FoV from the focal length alone,
    so the rasterizers' focal_x = W / (2 tanfovx) returns fx wherever the principal point is."""
    R = np.eye(3, dtype=np.float64) if R is None else np.asarray(R, dtype=np.float64)
    T = np.zeros(3, dtype=np.float64) if T is None else np.asarray(T, dtype=np.float64)
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    wvt = S.world2view(R, T).T.copy()
    Pm = np.zeros((4, 4), dtype=np.float32)
    Pm[0, 0] = 2.0 * fx / W
    Pm[1, 1] = 2.0 * fy / H
    Pm[0, 2] = 2.0 * cx / W - 1.0
    Pm[1, 2] = 2.0 * cy / H - 1.0
    Pm[3, 2] = 1.0
    Pm[2, 2] = zfar / (zfar - znear)
    Pm[2, 3] = -(zfar * znear) / (zfar - znear)
    full = (wvt.astype(np.float32) @ Pm.T).astype(np.float32)
    campos = np.linalg.inv(wvt.astype(np.float64))[3, :3].astype(np.float32)
    tanx, tany = W / (2.0 * fx), H / (2.0 * fy)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)
    return dict(W=W, H=H, FoVx=2.0 * math.atan(tanx), FoVy=2.0 * math.atan(tany), tanfovx=tanx, tanfovy=tany,
                viewmatrix=np.ascontiguousarray(wvt, dtype=np.float32), projmatrix=np.ascontiguousarray(full, dtype=np.float32),
                campos=campos, R=R.astype(np.float32), T=T.astype(np.float32), K=K, znear=znear, zfar=zfar)


# ------------------------------------------------------------------------------------------- the backward's image size
def backward_size(n, tanfov, dtype=np.float32):
    """The image extent the surfel backward rebuilds its homography for (DSR backward.cu:637-638, csrc/gsr_surfel.hip
    surfel_preprocess_bwd): int(focal * tan_fov * 2) with focal = n / (2 * tan_fov) formed on the host (csrc/gsr_internal.hpp make_cam),
    every operation in `dtype`.  tan_fov reaches the C ABI as a double and is converted to float there; the conversion is the first
    rounding.  In float32 the product is often one ulp under n and the result is n - 1."""
    t = dtype(tanfov)
    focal = dtype(n) / (dtype(2) * t)
    return int(focal * t * dtype(2))


def _fov_grid(lo_deg, hi_deg, step=0.05):
    return np.arange(lo_deg, hi_deg + 0.5 * step, step)


def focal_candidates(n, lo_deg=20.0, hi_deg=90.0, dtype=np.float32):
    """(focal, backward size) of every FoV on a 0.05 deg grid, the FoV passing through the focal length and back as in hwk_camera."""
    out = []
    for deg in _fov_grid(lo_deg, hi_deg):
        f = n / (2.0 * math.tan(math.radians(deg) / 2))
        out.append((f, backward_size(n, n / (2.0 * f), dtype)))
    return out


def trunc_search(W, H, ratio=1.0, dtype=np.float32):
    """Smallest (W', H') >= (W, H) (W' first) and focal lengths with backward_size == (W' - 1, H' - 1) and fx / fy within 10 % of `ratio`;
    also fy_keep, the nearest focal length to fy (a few ulps away) whose backward height stays H'.  Returns dict(W, H, fx, fy, fy_keep)."""
    for h in range(H, H + 16):
        ys = focal_candidates(h, dtype=dtype)
        ty = [f for f, b in ys if b == h - 1]
        for w in range(W, W + 16):
            tx = [f for f, b in focal_candidates(w, dtype=dtype) if b == w - 1]
            best = None
            for fy in ty:
                for fx in tx:
                    miss = abs(math.log(fx / fy / ratio))
                    if miss < math.log(1.1) and (best is None or miss < best[0]):
                        best = (miss, fx, fy)
            if best is not None:
                _, fx, fy = best
                # the sibling's fy: a few float32 ulps of the tangent away, so that nothing but the truncation tells the two cameras apart
                rel = float(np.finfo(dtype).eps)
                keep = next(f for k in range(1, 4096) for f in (fy * (1 + k * rel), fy * (1 - k * rel)) if backward_size(h, h / (2.0 * f), dtype) == h)
                return dict(W=w, H=h, fx=fx, fy=fy, fy_keep=keep)
    raise AssertionError("no truncating pair near %d x %d" % (W, H))


# ------------------------------------------------------------------------------------------- families
def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def rolled_pose(seed):
    """(R camera-to-world, T world-to-camera): roll 35 deg, pitch 12 deg, yaw -17 deg, each moved by up to 3 deg with the seed."""
    rs = np.random.RandomState(9000 + seed)
    j = rs.uniform(-3.0, 3.0, 3)
    w2c = _rot("z", 35.0 + j[0]) @ _rot("x", 12.0 + j[1]) @ _rot("y", -17.0 + j[2])
    return w2c.T, np.array([0.3, -0.2, 0.4]) + 0.05 * rs.randn(3)


def _offsets(W, H, seed):
    rs = np.random.RandomState(9100 + seed)
    sx, sy = (1.0 if seed & 1 else -1.0), (1.0 if seed & 2 else -1.0)
    return W / 2.0 + sx * rs.uniform(0.10, 0.20) * W, H / 2.0 + sy * rs.uniform(0.10, 0.20) * H


def _focal(n, fov_deg):
    return n / (2.0 * math.tan(math.radians(fov_deg) / 2))


def family(name, W, H, seed):
    ratio = 1.4 if seed % 2 == 0 else 1.0 / 1.4
    if name == "aniso":
        fy = _focal(H, 50.0)
        return hwk_camera(W, H, ratio * fy, fy, W / 2.0, H / 2.0)
    if name == "offcentre":
        f = _focal(H, 50.0)
        return hwk_camera(W, H, f, f, *_offsets(W, H, seed))
    if name == "rolled":
        f = _focal(H, 50.0)
        return hwk_camera(W, H, f, f, W / 2.0, H / 2.0, *rolled_pose(seed))
    if name in ("narrow", "wide"):
        f = _focal(H, 12.0 if name == "narrow" else 110.0)
        return hwk_camera(W, H, f, f, W / 2.0, H / 2.0)
    if name in ("trunc", "trunc_x"):
        t = trunc_search(W, H)
        return hwk_camera(t["W"], t["H"], t["fx"], t["fy"] if name == "trunc" else t["fy_keep"], t["W"] / 2.0, t["H"] / 2.0)
    if name == "all":
        t = trunc_search(W, H, ratio)
        return hwk_camera(t["W"], t["H"], t["fx"], t["fy"], *_offsets(t["W"], t["H"], seed), *rolled_pose(seed))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------- scenes
def frustum_scene(variant, P, cam, seed, overscan=1.6, sh_degree=3, bg=(0.0, 0.0, 0.0)):
    """kw for `cam`: view-space directions uniform over overscan x the FoV (about the optical axis); depths 0.15 .. 0.2 for NEAR_FRAC of
    the Gaussians (culled: the near plane is at 0.2) and log-uniform in 1 .. 8 for the rest.  Footprints 0.5 .. 6 px at the Gaussian's
    depth, axis ratios 1 .. 10 (S) or 1 .. 3 with a third scale of half the smaller one (G); 60 % of the Gaussians whose centre falls
    outside the image get a footprint of 0.4 .. 0.7 x their distance to it instead and face the camera, so that their 3-sigma rectangle
    reaches the image: those are the VISIBLE Gaussians beyond 1.3 x the FoV whose view-space position variant G clamps.
    (Why not closer and thinner: a first draft drew every depth log-uniformly from 0.15 and made the G splats up to fifty times flatter
    than wide.  Under `wide` the float32 oracle then missed the float64 oracle by 1.5e-2 of the max-norm of dL_drotations, all of it on
    clamped Gaussians a quarter of a unit from the camera: float32 cannot hold those gradients, whoever computes them.)"""
    rs = np.random.RandomState(seed)
    W, H = cam["W"], cam["H"]
    fx, fy, cx, cy = float(cam["K"][0, 0]), float(cam["K"][1, 1]), float(cam["K"][0, 2]), float(cam["K"][1, 2])
    z = np.where(rs.rand(P) < NEAR_FRAC, rs.uniform(0.15, 0.2, P), np.exp(rs.uniform(np.log(1.0), np.log(8.0), P)))
    u = rs.uniform(-1, 1, P) * overscan * cam["tanfovx"]
    v = rs.uniform(-1, 1, P) * overscan * cam["tanfovy"]
    p_view = np.stack([u * z, v * z, z], 1)
    V = cam["viewmatrix"].astype(np.float64)
    means = (p_view - V[3, :3]) @ np.linalg.inv(V[:3, :3])
    px, py = fx * u + cx - 0.5, fy * v + cy - 0.5
    dist = np.hypot(np.maximum(0, np.maximum(-px, px - (W - 1))), np.maximum(0, np.maximum(-py, py - (H - 1))))
    pix = np.exp(rs.uniform(np.log(0.5), np.log(6.0), P))
    reacher = (dist > 0) & (rs.rand(P) < 0.6)
    pix = np.where(reacher, np.maximum(pix, dist * rs.uniform(0.4, 0.7, P)), pix)
    # world size of a footprint of `pix` pixels: the projection Jacobian stretches a splat at the direction (u, v) by about
    # sqrt(1 + u^2 + v^2) (variant G evaluates it at the clamped direction), a factor of 3.5 in the corners of `wide`
    uc, vc = np.clip(u, -1.3 * cam["tanfovx"], 1.3 * cam["tanfovx"]), np.clip(v, -1.3 * cam["tanfovy"], 1.3 * cam["tanfovy"])
    r = pix * z / math.sqrt(fx * fy) / np.sqrt(1.0 + uc * uc + vc * vc)
    tang = np.stack([r, r * 10.0 ** -rs.uniform(0, 1.0 if variant == "S" else 0.5, P)], 1)
    tang = np.where((rs.rand(P) < 0.5)[:, None], tang, tang[:, ::-1])
    n = rs.randn(P, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    # the reaching splats face the camera to within about 40 degrees (an edge-on surfel tens of pixels wide has a rectangle of thousands)
    ray = -p_view / np.linalg.norm(p_view, axis=1, keepdims=True)
    facing = ray + 0.35 * n
    facing = (facing / np.linalg.norm(facing, axis=1, keepdims=True)) @ np.linalg.inv(V[:3, :3])
    n = np.where(reacher[:, None], facing, n)
    opac = np.where(reacher, rs.uniform(0.03, 0.3, P), rs.uniform(0.05, 1.0, P))
    thin = None if variant == "S" else 0.5 * tang.min(1, keepdims=True)
    sc = A._attributes(P, variant, rs, means, A._scales(variant, P, rs, tang, thin), A._rot_for_normal(n, rs), opac, n)
    return A._kw(variant, sc, cam, sh_degree, bg)


def clamp_classes(kw):
    """(in x, in y) bool [P]: the view-space position lies beyond 1.3 x the FoV, where variant G clamps it (float64 on the float32
    inputs: a Gaussian within rounding of the limit may be classed differently by the kernel, which the callers' counts of hundreds and
    gradient checks do not depend on — the clamp is continuous there)."""
    V = kw["viewmatrix"].astype(np.float64)
    t = kw["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    with np.errstate(all="ignore"):
        return np.abs(t[:, 0] / t[:, 2]) > 1.3 * kw["tanfovx"], np.abs(t[:, 1] / t[:, 2]) > 1.3 * kw["tanfovy"]


def view_of(cam, device="cuda"):
    """The view object render(), _settings, _ray_block and the reflection passes take, on the device, with the reference's
    HWK = (H, W, K) carrying the camera's own K; .ct holds the camera's arrays as tensors."""
    import torch
    tensors = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in cam.items() if isinstance(v, np.ndarray)}

    class View:
        ct = tensors
        FoVx, FoVy = cam["FoVx"], cam["FoVy"]
        image_width, image_height = cam["W"], cam["H"]
        world_view_transform, full_proj_transform, camera_center = tensors["viewmatrix"], tensors["projmatrix"], tensors["campos"]
        HWK, R, T = (cam["H"], cam["W"], cam["K"]), tensors["R"], tensors["T"]
        znear, zfar = cam["znear"], cam["zfar"]
    return View
