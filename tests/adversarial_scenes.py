"""Seeded scene families that reach the rarely taken branches of the tile kernels (the random box scenes of gsr_synth.make_scene
almost never do), and the float64 measure of how far each family reaches.

Every family returns the `kw` dict of helpers.scene_kwargs (plus the camera) for variant "S" (surfels) or "G" (3D Gaussians):
  surface    surfels on a sphere and three planes in the view of the C3 camera, normals along the surface normal, bimodal opacity
             sigmoid(N(+-3, 1)), log-normal scales with sigma 1 and 1 % of them x20: oblique, nearly edge-on splats on the floor and
             side wall, opaque layers that saturate mid-list.  Sized at any P (the spacing follows the surface area / P).
  grazing    splats whose normal makes 90 deg - {0, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 1} deg with the view ray, at pixel footprints of
             0.1..8 px, so that |p.z| of the forward's homography falls on both sides of the backward's 1e-6 and the forward's 1e-4.
             With transmat=True (variant S only) the precomputed homographies of every third splat contain the camera centre
             exactly (p.z == 0 at every pixel: _degenerate_transmats of test_gpu_eval_forward).
  threshold  opacities at float32(1/255), one ulp either side, 1.01/255, 0.5, 0.99, 0.995 and 1; axis ratios 1:10^k, k = 0..4 (G: 0..2);
             sub-pixel splats (the low-pass disc wins); centres on and +-0.5 px from 8-px block and 16-px tile borders; centres a few
             radii outside the image; depths at the near plane 0.2 and one ulp either side; discs reaching the camera plane.
  duplicates(kw) replaces the second half of any family by exact copies of the first half, as a clone step makes them: equal
             depth keys that the sorts must order by Gaussian index.

reach() measures what a family reaches from the float32 oracle's state, re-evaluating every (pixel, list entry) pair of the
forward in float64 numpy."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-splatting-reflection_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import gsr_synth as S  # noqa: E402

# (P, W, H, seed) of the scenes the GPU tests render (ragged sizes: partial tiles and 8x8 blocks at the right and bottom edges)
SCENES = {"surface": (3000, 200, 136, 5), "grazing": (3000, 200, 136, 6), "grazing_T": (3000, 200, 136, 7), "threshold": (3000, 200, 136, 8),
          "dup_surface": (3000, 232, 120, 9), "dup_threshold": (2400, 200, 136, 10)}
GRAZE_DEG = (0.0, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 1.0)
THRESH_OPACITIES = np.array([1 / 255, np.nextafter(np.float32(1 / 255), np.float32(0)), np.nextafter(np.float32(1 / 255), np.float32(1)),
                             1.01 / 255, 0.5, 0.99, 0.995, 1.0], np.float32)


# ------------------------------------------------------------------------------------------- geometry helpers
def _quat_from_frame(t1, t2, n):
    """Unit quaternions (r, x, y, z) of the rotations whose matrix has columns (t1, t2, n): the splat's tangent axes and normal
    (quat_to_rotmat of both rasterizers: scale axis k is column k)."""
    Rm = np.stack([t1, t2, n], axis=2)       # [N, 3 rows, 3 cols]
    m00, m11, m22 = Rm[:, 0, 0], Rm[:, 1, 1], Rm[:, 2, 2]
    tr = m00 + m11 + m22
    q = np.zeros((len(Rm), 4))
    c0 = tr > 0
    c1 = ~c0 & (m00 >= m11) & (m00 >= m22)
    c2 = ~c0 & ~c1 & (m11 >= m22)
    c3 = ~c0 & ~c1 & ~c2
    s = np.sqrt(np.maximum(tr + 1, 1e-30)) * 2
    q[c0] = np.stack([0.25 * s, (Rm[:, 2, 1] - Rm[:, 1, 2]) / s, (Rm[:, 0, 2] - Rm[:, 2, 0]) / s, (Rm[:, 1, 0] - Rm[:, 0, 1]) / s], 1)[c0]
    s = np.sqrt(np.maximum(1 + m00 - m11 - m22, 1e-30)) * 2
    q[c1] = np.stack([(Rm[:, 2, 1] - Rm[:, 1, 2]) / s, 0.25 * s, (Rm[:, 0, 1] + Rm[:, 1, 0]) / s, (Rm[:, 0, 2] + Rm[:, 2, 0]) / s], 1)[c1]
    s = np.sqrt(np.maximum(1 + m11 - m00 - m22, 1e-30)) * 2
    q[c2] = np.stack([(Rm[:, 0, 2] - Rm[:, 2, 0]) / s, (Rm[:, 0, 1] + Rm[:, 1, 0]) / s, 0.25 * s, (Rm[:, 1, 2] + Rm[:, 2, 1]) / s], 1)[c2]
    s = np.sqrt(np.maximum(1 + m22 - m00 - m11, 1e-30)) * 2
    q[c3] = np.stack([(Rm[:, 1, 0] - Rm[:, 0, 1]) / s, (Rm[:, 0, 2] + Rm[:, 2, 0]) / s, (Rm[:, 1, 2] + Rm[:, 2, 1]) / s, 0.25 * s], 1)[c3]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _frame(n, rs):
    """Random tangent frame (t1, t2) of unit normals n [N, 3], spun uniformly about n."""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    u = np.cross(n, a)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n, u)
    phi = rs.uniform(0, 2 * np.pi, len(n))[:, None]
    return np.cos(phi) * u + np.sin(phi) * v, -np.sin(phi) * u + np.cos(phi) * v


def _rot_for_normal(n, rs):
    t1, t2 = _frame(n, rs)
    return _quat_from_frame(t1, t2, n)


def _pixel_to_world(cam, px, py, z):
    """World point at view depth z seen at pixel (px, py) (inverse of the forward's ndc2pix for a camera with R = I, T = 0)."""
    fx = cam["W"] / (2.0 * cam["tanfovx"])
    fy = cam["H"] / (2.0 * cam["tanfovy"])
    return np.stack([(px - (cam["W"] - 1) / 2.0) * z / fx, (py - (cam["H"] - 1) / 2.0) * z / fy, z], -1)


def _attributes(P, variant, rs, means, scales, rots, opac, normals):
    shs = np.concatenate([rs.randn(P, 1, 3), 0.15 * rs.randn(P, 15, 3)], axis=1)
    refl = 1 / (1 + np.exp(2.0 - rs.randn(P, 1)))
    f = lambda x: np.ascontiguousarray(x, np.float32)
    sc = dict(means3D=f(means), scales=f(scales), rotations=f(rots), opacities=f(np.asarray(opac).reshape(P, 1)), shs=f(shs),
              refl_strengths=f(refl), env_scope_mask=np.ascontiguousarray(rs.rand(P) < 0.7))
    if variant == "G":
        sc["normals"] = f(normals)
        sc.pop("env_scope_mask")
    return sc


def _kw(variant, sc, cam, sh_degree, bg):
    W, H = cam["W"], cam["H"]
    kw = dict(bg=np.asarray(bg, np.float32), means3D=sc["means3D"], opacities=sc["opacities"], viewmatrix=cam["viewmatrix"],
              projmatrix=cam["projmatrix"], campos=cam["campos"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=H,
              image_width=W, sh_degree=sh_degree, shs=sc["shs"], refl_strengths=sc["refl_strengths"], scales=sc["scales"],
              rotations=sc["rotations"])
    if variant == "G":
        kw["normals"] = sc["normals"]
    else:
        kw["env_scope_mask"] = sc["env_scope_mask"]
    return kw


def _scales(variant, P, rs, tangent, thin=None):
    """[P, 2] (S) or [P, 3] (G: the third scale, along the normal, 0.2 x the smaller tangent scale) from tangent scales [P, 2].
    (Thinner G splats make the fp32 gradients of scales, rotations and means3D ill-conditioned: with a third scale of 1e-3 of the first
    their max-norm moved by up to 1e-3 between two GPU runs that differ only in the order of the float atomics, culling off against
    on; the bars of the suite cannot hold there for any summation order.)"""
    if variant == "S":
        return tangent
    thin = 0.2 * tangent.min(1, keepdims=True) if thin is None else thin
    return np.concatenate([tangent, thin], axis=1)


# ------------------------------------------------------------------------------------------- families
def surface(variant, P, W, H, seed, sh_degree=3, bg=(0.0, 0.0, 0.0)):
    """Sphere (centre (0.3, 0.1, 5), radius 1), floor y = 1.1, back wall z = 7.5 and side wall x = -2.2 in front of the C3 camera."""
    rs = np.random.RandomState(seed)
    cam = S.make_camera(W, H)
    parts = [("sphere", 4 * np.pi), ("floor", 5.0 * 5.5), ("back", 6.0 * 3.0), ("side", 2.2 * 5.0)]
    area = sum(a for _, a in parts)
    counts = [int(P * a / area) for _, a in parts]
    counts[0] += P - sum(counts)
    means, normals = [], []
    for (name, _), n in zip(parts, counts):
        if name == "sphere":
            d = rs.randn(n, 3)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            means.append(np.array([0.3, 0.1, 5.0]) + d)
            normals.append(d)
        elif name == "floor":
            means.append(np.stack([rs.uniform(-2.5, 2.5, n), np.full(n, 1.1), rs.uniform(2.5, 8.0, n)], 1))
            normals.append(np.tile([0.0, -1.0, 0.0], (n, 1)))
        elif name == "back":
            means.append(np.stack([rs.uniform(-3.0, 3.0, n), rs.uniform(-1.5, 1.5, n), np.full(n, 7.5)], 1))
            normals.append(np.tile([0.0, 0.0, -1.0], (n, 1)))
        else:
            means.append(np.stack([np.full(n, -2.2), rs.uniform(-1.2, 1.1, n), rs.uniform(3.0, 8.0, n)], 1))
            normals.append(np.tile([1.0, 0.0, 0.0], (n, 1)))
    means, normals = np.concatenate(means), np.concatenate(normals)
    perm = rs.permutation(P)
    means, normals = means[perm], normals[perm]
    mu = math.log(0.6 * math.sqrt(area / max(P, 1)))
    tang = np.exp(mu + 1.0 * rs.randn(P, 2))
    big = rs.rand(P) < 0.01
    tang[big] *= 20.0
    sc = _scales(variant, P, rs, tang)
    sign = np.where(rs.rand(P) < 0.5, -3.0, 3.0)
    opac = 1 / (1 + np.exp(-(sign + rs.randn(P))))
    sc = _attributes(P, variant, rs, means, sc, _rot_for_normal(normals, rs), opac, normals)
    return _kw(variant, sc, cam, sh_degree, bg), cam


def grazing(variant, P, W, H, seed, sh_degree=3, bg=(0.0, 0.0, 0.0), transmat=False):
    """Splats at random pixels and depths 2..6; normal at 90 deg - GRAZE_DEG[i % 7] to the view ray; footprint 0.1..8 px."""
    rs = np.random.RandomState(seed)
    cam = S.make_camera(W, H)
    z = rs.uniform(2.0, 6.0, P)
    means = _pixel_to_world(cam, rs.uniform(-4, W + 4, P), rs.uniform(-4, H + 4, P), z)
    v = means / np.linalg.norm(means, axis=1, keepdims=True)     # view ray (the camera sits at the origin)
    a = rs.randn(P, 3)
    u = a - (a * v).sum(1, keepdims=True) * v
    u /= np.linalg.norm(u, axis=1, keepdims=True)                # perpendicular to the ray
    th = np.radians(np.array(GRAZE_DEG))[np.arange(P) % len(GRAZE_DEG)]
    n = np.cos(th)[:, None] * u + np.sin(th)[:, None] * v
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    fy = H / (2.0 * cam["tanfovy"])
    # p.z of a pixel is (s1 f)(s2 f) (n . d): the product of the two axes' pixel footprints times the cosine between the normal and
    # the pixel's ray, a few 1e-3 one pixel off the line of an edge-on splat.  Footprints 0.1..8 px with axis ratios 1..10^-2.5 put
    # that product across 1e-6 and 1e-4 at the pixels around the centre, where the low-pass disc blends
    px_size = np.exp(rs.uniform(np.log(0.1), np.log(8.0), P))
    r = px_size * z / fy
    tang = np.stack([r, r * 10.0 ** -rs.uniform(0, 2.5, P)], 1)
    sc = _scales(variant, P, rs, tang)
    opac = rs.uniform(0.3, 1.0, P)
    sc = _attributes(P, variant, rs, means, sc, _rot_for_normal(n, rs), opac, n)
    kw = _kw(variant, sc, cam, sh_degree, bg)
    if transmat:
        assert variant == "S"
        kw = with_degenerate_transmats(kw, seed)
    return kw, cam


def with_degenerate_transmats(kw, seed, every=3):
    """The family with precomputed homographies (the oracle's own, so the rest of the scene is unchanged) in which every `every`-th
    splat plane contains the camera centre exactly: Tw = (0, 0, 1) and Tv.xy = Tu.xy / 2, so that p.z = 0 at every pixel."""
    from oracle import oracle as orc
    o = orc.SurfelOracle(np.float32)
    o.forward(**kw)
    T = o.state("transMat").reshape(-1, 9).copy()
    T[o.state("radii") == 0] = np.eye(3, dtype=np.float32).reshape(-1)      # culled surfels never wrote their T
    rs = np.random.RandomState(seed + 5)
    k = np.arange(0, len(T), every)
    a, b = rs.uniform(0.5, 3.0, len(k)), rs.uniform(0.5, 3.0, len(k))
    D = np.zeros((len(k), 9), np.float32)
    D[:, 0], D[:, 1], D[:, 2] = a, b, rs.uniform(0, kw["image_width"], len(k))
    D[:, 3], D[:, 4], D[:, 5] = 0.5 * a, 0.5 * b, rs.uniform(0, kw["image_height"], len(k))
    D[:, 8] = 1.0
    T[k] = D
    kw = dict(kw)
    kw["cov3D_precomp"] = np.ascontiguousarray(T, np.float32)
    kw["scales"] = kw["rotations"] = None
    return kw


def threshold(variant, P, W, H, seed, sh_degree=3, bg=(0.0, 0.0, 0.0)):
    """Every Gaussian sits on several thresholds at once: its opacity, axis ratio and placement class cycle with co-prime periods."""
    rs = np.random.RandomState(seed)
    cam = S.make_camera(W, H)
    i = np.arange(P)
    fy = H / (2.0 * cam["tanfovy"])
    # placement classes (period 7)
    cls = i % 7
    z = rs.uniform(2.0, 6.0, P)
    px, py = rs.uniform(0, W, P), rs.uniform(0, H, P)
    # 1, 2: on 8-px block / 16-px tile borders, or +-0.5 px from them
    step = np.where(cls == 1, 8, 16)
    off = rs.choice([-0.5, 0.0, 0.0, 0.5], P)
    bx = (np.floor(px / step) * step + off)
    by = (np.floor(py / step) * step + rs.choice([-0.5, 0.0, 0.0, 0.5], P))
    px = np.where((cls == 1) | (cls == 2), bx, px)
    py = np.where((cls == 1) | (cls == 2), by, py)
    # 3: centre a few radii outside the image
    side = rs.randint(0, 4, P)
    out = rs.uniform(2, 24, P)
    px = np.where((cls == 3) & (side == 0), -out, np.where((cls == 3) & (side == 1), W - 1 + out, px))
    py = np.where((cls == 3) & (side == 2), -out, np.where((cls == 3) & (side == 3), H - 1 + out, py))
    # 4: depth at the near plane 0.2 and one ulp either side
    near = np.array([0.2, np.nextafter(np.float32(0.2), np.float32(1)), np.nextafter(np.float32(0.2), np.float32(0)),
                     np.nextafter(np.nextafter(np.float32(0.2), np.float32(1)), np.float32(1))], np.float64)
    z = np.where(cls == 4, near[(i // 7) % 4], z)
    means = _pixel_to_world(cam, px, py, z)
    means[cls == 4, 2] = near[(i[cls == 4] // 7) % 4]          # exactly the float32 depth (R = I: p_view.z = z)
    # footprint in pixels: 5: sub-pixel (the low-pass disc wins); others 1..12 px
    pix = np.exp(rs.uniform(np.log(1.0), np.log(12.0), P))
    pix = np.where(cls == 5, rs.uniform(0.02, 0.4, P), pix)
    pix = np.where(cls == 4, rs.uniform(0.3, 3.0, P), pix)
    r = pix * z / fy
    ratio = 10.0 ** -((i // 3) % 5)                             # axis ratios 1:10^k (period 15 with the other axis)
    tang = np.stack([r, r * ratio], 1)
    tang = np.where(((i // 15) % 2 == 0)[:, None], tang, tang[:, ::-1])
    # 6: a disc reaching the camera plane (z 0.3..0.6, tangent extent 3 sigma > z, tilted towards the camera)
    n = rs.randn(P, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    reach_cam = cls == 6
    means[reach_cam] = _pixel_to_world(cam, rs.uniform(0, W, reach_cam.sum()), rs.uniform(0, H, reach_cam.sum()), rs.uniform(0.3, 0.6, reach_cam.sum()))
    tang[reach_cam] = np.stack([rs.uniform(0.3, 0.6, reach_cam.sum()), rs.uniform(0.005, 0.05, reach_cam.sum())], 1)
    n[reach_cam] = np.array([0.0, 0.0, -1.0]) + 0.8 * rs.randn(reach_cam.sum(), 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    if variant == "G":
        tang[:, 1] = np.maximum(tang[:, 1], 1e-2 * tang[:, 0])     # G: ratios down to 1:100 (see _scales)
        tang[:, 0] = np.maximum(tang[:, 0], 1e-2 * tang[:, 1])
    sc = _scales(variant, P, rs, tang)
    opac = THRESH_OPACITIES[i % len(THRESH_OPACITIES)]
    sc = _attributes(P, variant, rs, means, sc, _rot_for_normal(n, rs), opac, n)
    sc["opacities"] = np.ascontiguousarray(opac.reshape(P, 1))      # exact float32 values
    return _kw(variant, sc, cam, sh_degree, bg), cam


def duplicates(kw):
    """Second half = exact copies of the first half (every per-Gaussian input), as densify_and_clone makes them."""
    kw = dict(kw)
    P = kw["means3D"].shape[0]
    h = P // 2
    for k in ("means3D", "opacities", "shs", "refl_strengths", "scales", "rotations", "normals", "env_scope_mask", "cov3D_precomp"):
        if kw.get(k) is not None:
            a = np.array(kw[k], copy=True)
            a[P - h:] = a[:h]
            kw[k] = np.ascontiguousarray(a)
    return kw


def family(name, variant, P, W, H, seed, sh_degree=3, bg=(0.0, 0.0, 0.0)):
    """kw of a family by name; "dup_<family>" is duplicates() of that family."""
    if name.startswith("dup_"):
        return duplicates(family(name[4:], variant, P, W, H, seed, sh_degree, bg))
    if name == "grazing_T":
        return grazing(variant, P, W, H, seed, sh_degree, bg, transmat=True)[0]
    return {"surface": surface, "grazing": grazing, "threshold": threshold}[name](variant, P, W, H, seed, sh_degree, bg)[0]


# ------------------------------------------------------------------------------------------- reach
def reach(variant, kw, antialiasing=False):
    """Run the float32 oracle forward on kw and re-evaluate every (pixel, list entry) pair of its tile lists in float64 up to and
    including the pair that ends the pixel's list.  Counts:
      pz_lt_1e4 / pz_1e6_1e4   pairs with |p.z| < 1e-4 / 1e-6 <= |p.z| < 1e-4 that decide a pixel (S: the forward's grazing branch;
                               the second set is grazing in the forward only); pz_eq0 pairs with p.z == 0 exactly
      low_pass                 blending pairs in which the 2D low-pass term wins (rho2d < rho3d; S)
      alpha_edge               pairs with alpha in [1/255, 1.05/255]
      alpha_clamp              pairs with opacity * G >= 0.99 (the clamp)
      saturated                pixels whose list ends at the T < 1e-4 test before it runs out
      tied_keys                adjacent equal 64-bit (tile, depth) keys of the sorted list
      cam_plane                visible splats whose cutoff disc reaches the camera plane (S: the cull record's "always a hit")
      near_skip                pairs skipped by the per-pixel near-plane test (S)
      batch_pairs_gt32 / _gt48 share of (8x8 block, 64-entry batch) units of the backward with more than 32 / 48 (4x4 sub-block,
                               entry) blending pairs (S: the backward's batch cut at S_CAP)"""
    from oracle import oracle as orc
    W, H = int(kw["image_width"]), int(kw["image_height"])
    if variant == "S":
        o = orc.SurfelOracle(np.float32)
        o.forward(**kw)
        T = (kw["cov3D_precomp"] if kw.get("cov3D_precomp") is not None else o.state("transMat")).reshape(-1, 9).astype(np.float64)
        opa = o.state("normal_opacity")[:, 3].astype(np.float64)
    else:
        o = orc.GaussOracle(np.float32)
        o.forward(antialiasing=antialiasing, **kw)
        co = o.state("conic_opacity").astype(np.float64)
    m2d = o.state("means2D").astype(np.float64)
    radii = o.state("radii")
    pl = o.state("point_list").astype(np.int64)
    rg = o.state("ranges").astype(np.int64)
    keys = o.state("keys")
    last = o.state("n_contrib")
    last = (last[0] if variant == "S" else last).astype(np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    yy, xx = np.mgrid[0:16, 0:16]
    sub = (((yy // 8) * 2 + (xx // 8)) * 4 + ((yy % 8) // 4) * 2 + ((xx % 8) // 4)).reshape(-1)
    c = dict(pz_lt_1e4=0, pz_1e6_1e4=0, pz_eq0=0, low_pass=0, alpha_edge=0, alpha_clamp=0, saturated=0, near_skip=0, pairs=0, blended=0,
             batches=0, batch_pairs_gt32=0, batch_pairs_gt48=0)
    for tile in range(gx * gy):
        a, b = rg[tile]
        if b <= a:
            continue
        tx, ty = tile % gx, tile // gx
        PX, PY = (tx * 16 + xx).reshape(-1).astype(np.float64), (ty * 16 + yy).reshape(-1).astype(np.float64)
        inside = (PX < W) & (PY < H)
        lastp = np.where(inside, last[np.minimum(PY, H - 1).astype(int), np.minimum(PX, W - 1).astype(int)], 0)
        n = b - a
        ids = pl[a:b]
        with np.errstate(all="ignore"):
            dx, dy = m2d[ids, 0][:, None] - PX[None], m2d[ids, 1][:, None] - PY[None]
            if variant == "S":
                Tm = T[ids]
                Tu, Tv, Tw = Tm[:, 0:3], Tm[:, 3:6], Tm[:, 6:9]
                k = PX[None, :, None] * Tw[:, None, :] - Tu[:, None, :]
                l_ = PY[None, :, None] * Tw[:, None, :] - Tv[:, None, :]
                p = np.cross(k, l_)
                pz = np.abs(p[..., 2])
                unstable = pz < 1e-4
                sx, sy = np.where(unstable, 0, p[..., 0] / p[..., 2]), np.where(unstable, 0, p[..., 1] / p[..., 2])
                rho3 = np.where(unstable, 1e8, sx * sx + sy * sy)
                rho2 = 2.0 * (dx * dx + dy * dy)
                rho = np.minimum(rho3, rho2)
                depth = sx * Tw[:, None, 0] + sy * Tw[:, None, 1] + Tw[:, None, 2]
                near = depth < 0.2
                g = opa[ids][:, None] * np.exp(-0.5 * rho)
            else:
                q = co[ids, 0][:, None] * dx * dx + 2 * co[ids, 1][:, None] * dx * dy + co[ids, 2][:, None] * dy * dy
                rho = q
                near = np.zeros(q.shape, bool)
                g = co[ids, 3][:, None] * np.exp(-0.5 * q)
            alpha = np.minimum(0.99, g)
            blend = ~near & ~(-0.5 * rho > 0) & (alpha >= 1 / 255)
        e = np.arange(n)[:, None]
        # the entries a pixel's forward evaluates: up to its last contributor, plus the entry that ended the list by saturation
        seen = (e < lastp[None]) & inside[None]
        after = blend & (e >= lastp[None]) & inside[None]
        first_after = np.where(after.any(0), after.argmax(0), -1)
        sat = first_after >= 0
        c["saturated"] += int(sat.sum())
        seen |= (e == first_after[None]) & sat[None]
        c["pairs"] += int(seen.sum())
        c["blended"] += int((seen & blend).sum())
        c["alpha_edge"] += int((seen & blend & (alpha <= 1.05 / 255)).sum())
        c["alpha_clamp"] += int((seen & blend & (g >= 0.99)).sum())
        if variant == "S":
            c["pz_lt_1e4"] += int((seen & (pz < 1e-4)).sum())
            c["pz_1e6_1e4"] += int((seen & (pz >= 1e-6) & (pz < 1e-4)).sum())
            c["pz_eq0"] += int((seen & (pz == 0)).sum())
            c["low_pass"] += int((seen & blend & (rho2 < rho3)).sum())
            c["near_skip"] += int((seen & near).sum())
            # backward batches: (8x8 block, 64 entries) -> blending (4x4 sub-block, entry) pairs
            bl = seen & blend & (e < lastp[None])
            nb = (n + 63) // 64
            s_any = np.zeros((nb * 64, 16), bool)
            for s in range(16):
                s_any[:n, s] = bl[:, sub == s].any(1)
            per = s_any.reshape(nb, 64, 4, 4).sum(axis=(1, 3))       # batches x quadrants
            used = per > 0
            c["batches"] += int(used.sum())
            c["batch_pairs_gt32"] += int((per > 32).sum())
            c["batch_pairs_gt48"] += int((per > 48).sum())
    c["tied_keys"] = int((keys[1:] == keys[:-1]).sum())
    c["visible"] = int((radii > 0).sum())
    c["num_rendered"] = int(o.R)
    if variant == "S":
        vis = radii > 0
        Tw = T[:, 6:9]
        with np.errstate(all="ignore"):
            c2 = 2.0 * np.log(255.0 * opa) * 1.05 + 0.1       # the cull record's squared splat-space radius
        # sigma = Tw.x^2 + Tw.y^2 - Tw.z^2 / c2 >= 0: the disc u^2 + v^2 <= c2 reaches the camera plane
        c["cam_plane"] = int((vis & (opa >= 1 / 255) & (Tw[:, 0] ** 2 + Tw[:, 1] ** 2 - Tw[:, 2] ** 2 / c2 >= 0)).sum())
    return c
