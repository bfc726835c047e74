"""Small scenes for the forward tile kernels' vote against the pixels of a block that are still alive (tests/test_gpu_live_vote.py), built
splat by splat in pixel units in front of the fixed camera (R = I, T = 0), for both variants and for images of 40x24 px (whole tiles and
blocks only) and 41x23 px (a block column one pixel wide at the right edge, a block row seven pixels high at the bottom edge).

  stack     opaque patches over the left part of the image, three deep, in front of 170 large weak splats that reach every tile and 130 small
            ones: pixels retire inside the first batches of a list of more than 130 entries, the rest of their block goes on blending
  hole      an opaque layer that leaves one pixel of a block alive (one splat per pixel, three deep), then splats behind it: on the pixel, on
            other pixels of its block, and large ones over all of it.  At 41x23 the pixel sits in the block cut by both image edges
  cross     the same with one row and one column of the block left alive (the box of the live pixels stays the whole block while the mask
            changes), and splats behind that retire the middle of the row and of the column.  Both end with three opaque splats over the
            whole image and a few entries behind those
  rare      `stack` with grazing splats, splats whose cull record is unbounded (huge, or close to the camera plane) and splats that can
            never blend (opacity < 1/255)

retired_fraction() asks the oracle how many pixels have retired (T < 1e-4) before their tile's list ends; a scene is only worth running if many
have (tests/test_live_vote_scenes.py holds every scene to 25 %)."""
import numpy as np

import adversarial_scenes as A
from helpers import S

SIZES = [(40, 24), (41, 23)]
NAMES = ["stack", "hole", "cross", "rare"]


class _Splats:
    """Splats given by the pixel they sit on, their view depth, their footprint (standard deviations along their two axes, in pixels),
    their opacity and their normal (None: facing the camera)."""

    def __init__(self, cam):
        self.cam, self.rows = cam, []
        self.fy = cam["H"] / (2.0 * cam["tanfovy"])

    def add(self, px, py, z, sig, opac, normal=None):
        px, py, z, opac = np.broadcast_arrays(*[np.asarray(v, np.float64) for v in (px, py, z, opac)])
        n = len(px)
        sig = np.broadcast_to(np.asarray(sig, np.float64).reshape(-1, 1) if np.ndim(sig) < 2 else sig, (n, 2))
        nrm = np.tile([0.0, 0.0, -1.0], (n, 1)) if normal is None else normal
        self.rows.append((A._pixel_to_world(self.cam, px, py, z), sig * z[:, None] / self.fy, nrm, opac))

    def kw(self, variant, seed, sh_degree=1):
        rs = np.random.RandomState(seed)
        means, tang, nrm, opac = [np.concatenate([r[i] for r in self.rows]) for i in range(4)]
        P = len(means)
        sc = A._attributes(P, variant, rs, means, A._scales(variant, P, rs, tang), A._rot_for_normal(nrm, rs), opac, nrm)
        kw = A._kw(variant, sc, self.cam, sh_degree, (0.1, 0.2, 0.3))
        kw["shs"] = np.ascontiguousarray(kw["shs"][:, :(sh_degree + 1) ** 2])
        return kw


def _opaque_patches(sp, xs, ys, z0, layers=3, sig=2.5):
    """Opaque splats (alpha 0.99 at their centre) on the grid xs x ys, `layers` deep."""
    gx, gy = np.meshgrid(xs, ys)
    for k in range(layers):
        sp.add(gx.ravel(), gy.ravel(), z0 + 0.05 * k, sig, 1.0)


def _pixel_layer(sp, pixels, z0, layers=3):
    """One tiny opaque splat per pixel of `pixels` [N, 2], `layers` deep: retires those pixels and multiplies their neighbours' T by 0.1 .. 0.2 a layer."""
    for k in range(layers):
        sp.add(pixels[:, 0], pixels[:, 1], z0 + 0.05 * k, 0.3, 1.0)


def stack(variant, W, H, seed):
    rs = np.random.RandomState(seed)
    sp = _Splats(S.make_camera(W, H))
    _opaque_patches(sp, np.arange(2.0, 0.7 * W, 5.0), np.arange(2.0, H, 5.0), 2.0, layers=4)
    n = 170                                            # large and weak: every tile's list grows past two batches
    sp.add(rs.uniform(0, W, n), rs.uniform(0, H, n), rs.uniform(3.0, 6.0, n), rs.uniform(3.0, 5.0, (n, 2)), rs.uniform(0.04, 0.2, n))
    n = 130                                            # small: many reach only the retired part of a block
    sp.add(rs.uniform(0, W, n), rs.uniform(0, H, n), rs.uniform(3.0, 6.0, n), rs.uniform(0.5, 1.5, (n, 2)), rs.uniform(0.1, 0.6, n))
    return sp


def _masked_block(variant, W, H, seed, bx, by, alive):
    """The block at (bx, by) with only the pixels `alive` (offsets inside the block) left alive: a per-pixel opaque layer over the rest of
    the block and a margin of one pixel around it."""
    rs = np.random.RandomState(seed)
    sp = _Splats(S.make_camera(W, H))
    keep = {(bx + i, by + j) for i, j in alive}
    win = [(x, y) for x in range(bx - 1, bx + 9) for y in range(by - 1, by + 9) if 0 <= x < W and 0 <= y < H and (x, y) not in keep]
    _pixel_layer(sp, np.asarray(win, np.float64), 2.0)
    return sp, rs, sorted(keep)


def _close(sp, rs, W, H):
    """Behind everything else: three opaque splats over the whole image, which retire every pixel that is left, and a few more entries, so
    that no list ends where its pixels retire."""
    sp.add([W / 2.0] * 3, [H / 2.0] * 3, [8.0, 8.1, 8.2], 400.0, 1.0)
    sp.add(rs.uniform(0, W, 16), rs.uniform(0, H, 16), rs.uniform(9.0, 10.0, 16), 5.0, rs.uniform(0.1, 0.5, 16))


def hole(variant, W, H, seed):
    bx, by = (40, 16) if W % 8 else (16, 8)            # 41x23: the block cut by the right and the bottom image edge (one column, seven rows)
    off = (0, 4) if W % 8 else (3, 4)
    sp, rs, keep = _masked_block(variant, W, H, seed, bx, by, [off])
    (hx, hy), = keep
    n = 24
    # behind the layer: small splats on the live pixel, small splats on other pixels of the block, and large ones over the whole block
    sp.add(np.full(n, hx) + rs.uniform(-0.4, 0.4, n), np.full(n, hy) + rs.uniform(-0.4, 0.4, n), rs.uniform(3.0, 4.0, n), 0.5, rs.uniform(0.1, 0.6, n))
    ox, oy = rs.randint(0, 8, n), rs.randint(0, 8, n)
    far = np.maximum(np.abs(bx + ox - hx), np.abs(by + oy - hy)) >= 3
    sp.add((bx + ox)[far], (by + oy)[far], rs.uniform(3.0, 4.0, int(far.sum())), 0.4, rs.uniform(0.3, 0.9, int(far.sum())))
    sp.add(bx + rs.uniform(0, 8, n), by + rs.uniform(0, 8, n), rs.uniform(4.0, 5.0, n), rs.uniform(3.0, 6.0, (n, 2)), rs.uniform(0.05, 0.3, n))
    _close(sp, rs, W, H)
    return sp


def cross(variant, W, H, seed):
    bx, by = (32, 16) if W % 8 else (16, 8)            # 41x23: a block cut by the bottom edge (its last row is outside the image)
    row, col = 2, 5
    alive = [(i, row) for i in range(8)] + [(col, j) for j in range(8)]
    sp, rs, keep = _masked_block(variant, W, H, seed, bx, by, alive)
    # behind the layer: opaque splats that retire the middle of the row and of the column, one pixel at a time, the ends stay alive
    mid = [(bx + i, by + row) for i in range(2, 6)] + [(bx + col, by + j) for j in range(3, 6)]
    for k, (x, y) in enumerate(mid):
        for d in range(3):
            sp.add([x], [y], [3.0 + 0.2 * k + 0.05 * d], 0.3, 1.0)
    n = 40
    sp.add(bx + rs.uniform(-2, 10, n), by + rs.uniform(-2, 10, n), rs.uniform(5.0, 6.0, n), rs.uniform(0.5, 4.0, (n, 2)), rs.uniform(0.05, 0.5, n))
    _close(sp, rs, W, H)
    return sp


def rare(variant, W, H, seed):
    rs = np.random.RandomState(seed + 1)
    sp = stack(variant, W, H, seed)
    n = 30
    # grazing: the normal 0.02 .. 2 degrees off perpendicular to the view ray (adversarial_scenes.grazing)
    z = rs.uniform(3.0, 6.0, n)
    px, py = rs.uniform(0, W, n), rs.uniform(0, H, n)
    v = A._pixel_to_world(sp.cam, px, py, z)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    a = rs.randn(n, 3)
    u = a - (a * v).sum(1, keepdims=True) * v
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    th = np.radians(np.array([0.0, 0.02, 0.1, 0.5, 2.0]))[np.arange(n) % 5]
    nrm = np.cos(th)[:, None] * u + np.sin(th)[:, None] * v
    sp.add(px, py, z, np.stack([rs.uniform(2.0, 8.0, n), rs.uniform(0.05, 2.0, n)], 1), rs.uniform(0.3, 1.0, n), nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    # unbounded cull records: footprints far larger than the image, and splats that straddle the camera plane
    sp.add(rs.uniform(0, W, 6), rs.uniform(0, H, 6), rs.uniform(4.0, 6.0, 6), 4000.0, rs.uniform(0.02, 0.1, 6))
    zc = np.full(6, 0.25)
    tilt = np.tile([0.0, 0.8, -0.6], (6, 1))
    sp.add(rs.uniform(0, W, 6), rs.uniform(0, H, 6), zc, 60.0, rs.uniform(0.02, 0.1, 6), tilt)
    # never blends
    sp.add(rs.uniform(0, W, 12), rs.uniform(0, H, 12), rs.uniform(2.2, 6.0, 12), 3.0, 0.003)
    return sp


BUILDERS = dict(stack=stack, hole=hole, cross=cross, rare=rare)


def scene(name, variant, W, H, seed=7):
    return BUILDERS[name](variant, W, H, seed).kw(variant, seed)


def empty(variant, W, H):
    """P = 0."""
    kw = scene("stack", variant, W, H)
    for k in ("means3D", "opacities", "shs", "refl_strengths", "scales", "rotations", "normals", "env_scope_mask"):
        if k in kw:
            kw[k] = np.ascontiguousarray(kw[k][:0])
    return kw


def _oracle(variant):
    from oracle import oracle as orc
    return (orc.SurfelOracle if variant == "S" else orc.GaussOracle)(np.float32)


def retired_fraction(name, variant, W, H, seed=7):
    """(share of the image's pixels that retire before their tile's list ends, longest tile list) by the oracle.  A probe splat far behind
    the scene, over the whole image, with alpha 0.05 is the last entry of every tile's list and blends into exactly the pixels that are
    still alive there (T >= 1e-4 leaves 0.95 T >= 0.95e-4: it may retire a pixel within 5 % of the threshold instead, which then counts
    as retired before the end), so the oracle's last contributor tells the two apart."""
    sp = BUILDERS[name](variant, W, H, seed)
    sp.add([W / 2.0], [H / 2.0], [50.0], 400.0, 0.05)
    kw = sp.kw(variant, seed)
    o = _oracle(variant)
    o.forward(**kw)
    last = o.state("n_contrib").reshape(-1, H, W)[0].astype(np.int64)
    rg = o.state("ranges").astype(np.int64).reshape(-1, 2)
    count = (rg[:, 1] - rg[:, 0]).reshape((H + 15) // 16, (W + 15) // 16)
    per_px = np.repeat(np.repeat(count, 16, axis=0), 16, axis=1)[:H, :W]
    assert (last <= per_px).all()
    return float((last < per_px).mean()), int(count.max()) - 1
