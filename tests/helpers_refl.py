"""Pixel-exact inputs for the deferred reflection and a float64 classifier of its cubemap lookup (test infrastructure only).

make_targets() solves, pixel by pixel, the `normal_view` that makes reference_chain (tests/helpers_chain.py) reflect the pixel's view ray
onto a chosen direction r*: an interior texel cell, one of the 24 face-edge rim strips, one of the 24 face-corner vertex squares, an exact
face centre, cube edge or cube vertex, plus zero and tiny normals and (optionally) a band of random ones.

classify() restates the reference's face choice and texel coordinates (CME cubemapencoder.cu:147-263, as oracle/oracle_cubemap.cpp) in
float64 and returns each direction's lookup class and its MARGIN: the distance, in texel units, to the nearest discontinuity of the lookup.
The lookup is continuous in the direction, but which texels it reads and with which slope is not; its discontinuities are
  * the half-integer cell borders lu, lv = k + 1/2 (the floor in Compute_Seamless_Index),
  * the rim thresholds 0.5 and L - 0.5 (which of the edge-table branches runs; they are cell borders too),
  * the face-choice tie |major| = |second| (lu or lv = 0 or L).

Ambiguity bound.  The kernels compute the reflected direction r in float32 from the float32 inputs the float64 chain is evaluated on:
about ten roundings of unit-scale quantities (rotation, K^-1 product, ray normalisation, d.n, r = d - 2 n d.n) and, in the default build,
the 1-ulp hardware v_rcp / v_rsq / v_sqrt.  |dr|_inf <= 16 * 2^-24 = 2^-20 covers that with room.  The lookup divides by the major
component m (|m| >= |r|/sqrt(3), |a| <= |m|):  |du| <= (|da| + |u| |dm|) / |m| + ulp <= 2 sqrt(3) 2^-20 / |r| + 2^-23, and lu = (u/2 + 1/2) L
adds two roundings of size ulp(L):  |dlu| <= (sqrt(3) 2^-20 / |r| + 2^-22) L < 2^-19 L / min(1, |r|).
DELTA(L) = 2^-16 L is 8x that bound; classify() reports the margin multiplied by min(1, |r|) (|r| < 1 only for normals so short that the
+1e-6 of the normalisation shrinks them), so that `margin < DELTA` is the one test for every pixel.  A pixel whose margin is below DELTA is
AMBIGUOUS: float32 may put it on the other side of the discontinuity.  The targets of every class except the exact edges and vertices
(and the exact face centres at odd L, where L/2 is a cell border) are placed at margin >= 8 DELTA and land at >= 4 DELTA.
"""
import os

import numpy as np
import torch

from helpers import S               # (puts the repository and the package on sys.path)
from helpers_chain import reference_dirs

EPS_N = 1e-6           # gaussian_renderer/__init__.py:179 of the reference: n / (|n| + 1e-6)

# lookup classes
FAIL, INTERIOR, RIM, VERTEX = 0, 1, 2, 3
# target kinds
K_INTERIOR, K_BORDER, K_RIM, K_VERTEX, K_CENTRE, K_EDGE, K_CORNER, K_ZERO, K_TINY, K_RANDOM = range(10)
KIND_NAMES = ["interior", "near_border", "rim", "vertex", "face_centre", "exact_edge", "exact_vertex", "zero_normal", "tiny_normal", "random"]
AMBIGUOUS_KINDS = (K_EDGE, K_CORNER)     # (and K_CENTRE at odd L)
RIM_PER_EDGE = 20      # pixels per face-edge rim strip and per face-corner vertex square (the issue asks for >= 16)


def delta(L):
    """Ambiguity margin in texel units (derivation in the module docstring)."""
    return 2.0 ** -16 * L


def cube_coords(r, L):
    """float64 CME Compute_Cubemap_UV + the texel coordinates of Compute_Seamless_Index: (face, lu, lv, u, v) for directions r [N,3]."""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    dim = np.argmax(a, axis=1)       # first maximal component, as the reference's strict `>` comparisons
    N = r.shape[0]
    m = r[np.arange(N), dim]
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(dim == 0, z / x, np.where(dim == 1, x / y, x / z))
        v = np.where(dim == 0, y / x, np.where(dim == 1, z / y, y / z))
    face = 2 * dim + (m < 0)
    u = np.where((face == 0) | (face == 1) | (face == 3), -u, u)
    v = np.where((face == 0) | (face == 3) | (face == 4), -v, v)
    lu = (u * 0.5 + 0.5) * L
    lv = (-v * 0.5 + 0.5) * L
    return face, lu, lv, u, v


def direction_of(face, lu, lv, L):
    """Inverse of cube_coords (a direction, not normalised, with major component +-1).  lu / lv beyond [0, L] continue the face's plane
    and so reach the neighbouring faces."""
    face = np.asarray(face)
    u = 2.0 * np.asarray(lu, np.float64) / L - 1.0
    v = 1.0 - 2.0 * np.asarray(lv, np.float64) / L
    one = np.ones_like(u)
    table = {0: (one, -v, -u), 1: (-one, -v, u), 2: (u, one, v), 3: (u, -one, v), 4: (u, -v, one), 5: (-u, -v, -one)}
    out = np.zeros(u.shape + (3,))
    for f, comps in table.items():
        sel = face == f
        out[sel] = np.stack([c[sel] for c in comps], axis=-1)
    return out


def classify(r, L):
    """(class [N], face [N], flag [N], margin [N], lu [N], lv [N]) of reflected directions r [N,3] (float64).  flag as the kernel's
    Seamless::flag: 1 lu < 0.5, 2 lu >= L - 0.5, 4 lv < 0.5, 8 lv >= L - 0.5.  margin: texel distance to the nearest discontinuity times
    min(1, |r|) (module docstring); +inf for the fail direction r = 0 (it has no neighbours)."""
    r = np.asarray(r, np.float64)
    face, lu, lv, _, _ = cube_coords(r, L)
    flag = np.where(lu < 0.5, 1, np.where(lu >= L - 0.5, 2, 0)) | np.where(lv < 0.5, 4, np.where(lv >= L - 0.5, 8, 0))
    cell = lambda t: np.abs(t - 0.5 - np.clip(np.round(t - 0.5), 0, L - 1))
    tie = np.minimum(np.minimum(lu, L - lu), np.minimum(lv, L - lv))
    margin = np.minimum(np.minimum(cell(lu), cell(lv)), tie) * np.minimum(1.0, np.linalg.norm(r, axis=1))
    fail = ~np.any(r != 0, axis=1)
    hu, hv = (flag & 3) != 0, (flag & 12) != 0
    cls = np.where(fail, FAIL, np.where(hu & hv, VERTEX, np.where(hu | hv, RIM, INTERIOR)))
    margin = np.where(fail, np.inf, margin)
    return cls, face, flag, margin, lu, lv


def edge_id(face, flag):
    """0..23 for a rim pixel: face * 4 + (0: lu < 0.5, 1: lu >= L - 0.5, 2: lv < 0.5, 3: lv >= L - 0.5)."""
    side = np.where(flag & 1, 0, np.where(flag & 2, 1, np.where(flag & 4, 2, 3)))
    return face * 4 + side


def corner_id(face, flag):
    """0..23 for a vertex pixel: face * 4 + 2 * (lv side) + (lu side)."""
    return face * 4 + 2 * ((flag & 8) != 0) + ((flag & 2) != 0)


def camera_mats(cam):
    """world_view_transform[:3,:3] as reference_chain applies it to a column vector: rn = M @ n_view."""
    return np.asarray(cam["viewmatrix"], np.float32).astype(np.float64)[:3, :3]


def view_rays(cam, W, H):
    """The reference chain's unit view ray of every pixel, [H*W, 3] float64."""
    _, rd, _ = reference_dirs(torch.zeros(3, H, W, dtype=torch.float64), cam, W, H)
    return rd.reshape(-1, 3).numpy()


def solve_normals(cam, d, rstar, length):
    """View-space normals of length `length` [N] whose reference chain reflects the unit rays d [N,3] onto the direction of rstar [N,3].
    With n_world = length * nhat the chain normalises to lam nhat, lam = length / (length + 1e-6), and reflects to
    r = d - 2 lam^2 (d.nhat) nhat = (1 - lam^2) d + lam^2 t, where t is the mirror image of d in the plane of nhat (nhat ~ d - t).
    t is picked on the unit circle through d and r* so that r is parallel to r*:  t = (mu r* - a d) / lam^2, a = 1 - lam^2,
    mu = a (r*.d) + sqrt(a^2 (r*.d)^2 - a^2 + lam^4).  The view-space normal inverts the rotation reference_chain applies."""
    d = np.asarray(d, np.float64)
    rs = np.asarray(rstar, np.float64)
    rs = rs / np.linalg.norm(rs, axis=1, keepdims=True)
    length = np.asarray(length, np.float64)
    lam2 = (length / (length + EPS_N)) ** 2
    a = 1.0 - lam2
    c = (rs * d).sum(1)
    mu = a * c + np.sqrt(np.maximum(a * a * c * c - a * a + lam2 * lam2, 0.0))
    t = (mu[:, None] * rs - a[:, None] * d) / lam2[:, None]
    nw = d - t
    nw = nw / np.linalg.norm(nw, axis=1, keepdims=True) * length[:, None]
    return np.linalg.solve(camera_mats(cam), nw.T).T


def chain_dirs(nv, cam, W, H):
    """Reflected directions [H*W,3] of reference_chain on the float32 normal_view nv [3,H,W] (evaluated in float64)."""
    _, _, r = reference_dirs(torch.from_numpy(np.asarray(nv, np.float32)).double(), cam, W, H)
    return r.reshape(-1, 3).numpy()


def _coord_interior(rng, n, L, m, near_border=False):
    """Texel coordinates k + 1/2 + f inside the rim (L >= 2), at >= m from every cell border; near_border: f within m..m+1/32 of one."""
    k = rng.integers(0, L - 1, n)
    if near_border:
        f = m + rng.random(n) / 32
        f = np.where(rng.random(n) < 0.5, f, 1.0 - f)
    else:
        f = m + rng.random(n) * (1 - 2 * m)
    return k + 0.5 + f


def _coord_rim(rng, n, L, m, hi):
    """A coordinate inside the half-texel rim strip, at >= m from the threshold and from the face-choice tie."""
    t = m + rng.random(n) * (0.5 - 2 * m)
    return np.where(hi, L - t, t)


def make_targets(cam, W, H, L, seed, random_band=True):
    """Per-pixel targets for one image.  Returns dict(nv=float32 [3,H,W], kind=int [H*W], want=int [H*W] (the intended edge / corner id for
    rim / vertex kinds, else -1)).  Kinds are scattered over the image in random order (so that rim pixels share waves and tiles with
    interior ones).  Without random_band the pixels left over are interior targets."""
    rng = np.random.default_rng(seed)
    N = W * H
    m = 8 * delta(L)
    d = view_rays(cam, W, H)
    _, _, _, dmargin, _, _ = classify(d, L)
    kind = np.full(N, K_RANDOM if random_band else K_INTERIOR)
    want = np.full(N, -1)
    plan = []
    if L >= 2:
        plan += [(K_RIM, e) for e in range(24) for _ in range(RIM_PER_EDGE)]
    plan += [(K_VERTEX, c) for c in range(24) for _ in range(RIM_PER_EDGE)]
    plan += [(K_CENTRE, f) for f in range(6) for _ in range(4)]
    plan += [(K_EDGE, e) for e in range(12) for _ in range(4)]
    plan += [(K_CORNER, c) for c in range(8) for _ in range(4)]
    plan += [(K_TINY, -1)] * 128
    if L >= 2:
        plan += [(K_INTERIOR, -1)] * 1200 + [(K_BORDER, -1)] * 1200
    # zero normals (r = d) on pixels whose own view ray is unambiguous
    zero_px = rng.permutation(np.nonzero(dmargin >= 4 * delta(L))[0])[:64]
    free = rng.permutation(np.setdiff1d(np.arange(N), zero_px))
    assert len(plan) <= len(free), "image too small for the targets"
    px = free[:len(plan)]
    kind[zero_px] = K_ZERO
    kind[px] = [k for k, _ in plan]
    want[px] = [w for _, w in plan]
    rstar = np.zeros((N, 3))
    face = rng.integers(0, 6, N)
    # interior cells (L >= 2)
    for k, nb in ((K_INTERIOR, False), (K_BORDER, True)):
        s = kind == k
        n = int(s.sum())
        if n:
            lu, lv = _coord_interior(rng, n, L, m, nb), _coord_interior(rng, n, L, m)
            if nb:      # the near-border coordinate is lu or lv at random (or both)
                sw = rng.integers(0, 3, n)
                lu, lv = np.where(sw == 1, lv, lu), np.where(sw == 1, lu, np.where(sw == 2, _coord_interior(rng, n, L, m, True), lv))
            rstar[s] = direction_of(face[s], lu, lv, L)
    s = kind == K_RIM
    if s.any():
        e = want[s]
        f, side = e // 4, e % 4
        n = int(s.sum())
        rim = _coord_rim(rng, n, L, m, side % 2 == 1)
        other = _coord_interior(rng, n, L, m)
        lu = np.where(side < 2, rim, other)
        lv = np.where(side < 2, other, rim)
        rstar[s] = direction_of(f, lu, lv, L)
    s = kind == K_VERTEX
    if s.any():
        c = want[s]
        f, cu, cv = c // 4, c % 2, (c % 4) // 2
        n = int(s.sum())
        rstar[s] = direction_of(f, _coord_rim(rng, n, L, m, cu == 1), _coord_rim(rng, n, L, m, cv == 1), L)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    edges = np.array([[sa, sb, 0] for sa in (1, -1) for sb in (1, -1)] + [[sa, 0, sb] for sa in (1, -1) for sb in (1, -1)] +
                     [[0, sa, sb] for sa in (1, -1) for sb in (1, -1)], np.float64)
    corners = np.array([[sa, sb, sc] for sa in (1, -1) for sb in (1, -1) for sc in (1, -1)], np.float64)
    for k, tab in ((K_CENTRE, axes), (K_EDGE, edges), (K_CORNER, corners)):
        s = kind == k
        rstar[s] = tab[want[s]]
    want[(kind == K_CENTRE) | (kind == K_EDGE) | (kind == K_CORNER)] = -1
    # view-space normals: random length in [0.3, 1] for the targets, as the issue asks
    length = 0.3 + 0.7 * rng.random(N)
    nv = np.zeros((N, 3))
    tgt = (kind != K_RANDOM) & (kind != K_ZERO) & (kind != K_TINY)
    nv[tgt] = solve_normals(cam, d[tgt], rstar[tgt], length[tgt])
    s = kind == K_RANDOM
    g = rng.standard_normal((int(s.sum()), 3))
    nv[s] = g / np.linalg.norm(g, axis=1, keepdims=True) * length[s, None]
    # tiny normals |n| in [1e-7, 1e-4] (the +1e-6 of the normalisation and the len > 0 branch), redrawn until unambiguous
    s = np.nonzero(kind == K_TINY)[0]
    tl = 10.0 ** rng.uniform(-7, -4, len(s))
    todo = s
    for _ in range(50):
        g = rng.standard_normal((len(todo), 3))
        nv[todo] = g / np.linalg.norm(g, axis=1, keepdims=True) * tl[np.searchsorted(s, todo), None]
        img = nv.T.reshape(3, H, W).astype(np.float32)
        _, _, _, mg, _, _ = classify(chain_dirs(img, cam, W, H)[todo], L)
        todo = todo[mg < 4 * delta(L)]
        if len(todo) == 0:
            break
    assert len(todo) == 0
    return dict(nv=np.ascontiguousarray(nv.T.reshape(3, H, W).astype(np.float32)), kind=kind, want=want)


def classify_image(nv, cam, W, H, L):
    """classify() of the reference chain's reflected directions for the float32 normal_view nv [3,H,W]."""
    return classify(chain_dirs(nv, cam, W, H), L)


def pushed_normals(nv, cam, W, H, L, pix):
    """For the pixels `pix`: view-space normals (same length) whose reference direction is the pixel's own one moved by (du, dv) texels in
    its face's plane, for du in {-1/4, 0, 1/4} DELTA and dv in {-1/2, 0, 1/2} DELTA (unequal, so that a push off a cube vertex leaves the
    three-way tie by DELTA/4).  The kernels' texel coordinates are within 2^-19 L = DELTA/8 of the float64 ones (module docstring), so every
    discontinuity the kernel can end up beyond is crossed by one of the pushes, and a push overshoots the kernel's point by at most
    DELTA/2 + DELTA/8: the per-pixel gradient moves by DELTA times its own size over that, the floor of outside_envelope.  Returns a list
    of eight float32 [3,H,W] images that differ from nv on `pix` only."""
    r = chain_dirs(nv, cam, W, H)
    face, lu, lv, _, _ = cube_coords(r[pix], L)
    d = view_rays(cam, W, H)[pix]
    flat = np.asarray(nv, np.float32).reshape(3, -1)
    length = np.linalg.norm(flat[:, pix].astype(np.float64), axis=0)
    # A zero normal cannot move its direction (r = d) and needs no push: its normal gradient does not depend on the lookup
    # (g_n = -2 [(d.n) g_r + (g_r.n) d] = 0 at n = 0) and its forward output is continuous in the direction.
    moved = length > 0
    pix, face, lu, lv, d, length = pix[moved], face[moved], lu[moved], lv[moved], d[moved], length[moved]
    dl = delta(L)
    out = []
    for du in (-dl / 4, 0.0, dl / 4):
        for dv in (-dl / 2, 0.0, dl / 2):
            if du == 0 and dv == 0:
                continue
            img = flat.copy()
            n = solve_normals(cam, d, direction_of(face, lu + du, lv + dv, L), length).T
            # n and -n reflect alike but their gradients have opposite signs: keep the pixel's own orientation
            n *= np.where((n * flat[:, pix]).sum(axis=0) < 0, -1.0, 1.0)[None]
            img[:, pix] = n.astype(np.float32)
            out.append(img.reshape(3, H, W))
    return out


# ---------------------------------------------------------------------------------------------- inputs, float64 reference, HIP paths, checks
SEAM_W, SEAM_H = 157, 93          # odd pixel count, ragged 16x16 tiles on both axes


def seam_camera(W=SEAM_W, H=SEAM_H):
    return S.look_at_camera(W, H, eye=(1.0, -0.5, -4.0))


def seam_inputs(L, seed, W=SEAM_W, H=SEAM_H, cam=None):
    """The targeted image of make_targets plus random base colour, strength, cubemap, fail value and upstream weights; `amb` marks the
    ambiguous pixels (margin < DELTA).  cam: another camera of size W x H than seam_camera's."""
    cam = seam_camera(W, H) if cam is None else cam
    t = make_targets(cam, W, H, L, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    inp = dict(L=L, W=W, H=H, cam=cam, nv=t["nv"], kind=t["kind"],
               base=torch.rand(3, H, W, generator=g).numpy(), strength=torch.rand(1, H, W, generator=g).numpy(),
               tex=(torch.rand(6, 3, L, L, generator=g) - 0.5).numpy(), fail=(torch.randn(3, generator=g) * 0.5).numpy(),
               wf=torch.randn(3, H, W, generator=g).numpy(), wc=torch.randn(3, H, W, generator=g).numpy(),
               wn=torch.randn(3, H, W, generator=g).numpy())
    cls, face, flag, margin, _, _ = classify_image(t["nv"], cam, W, H, L)
    inp.update(cls=cls, margin=margin, amb=margin < delta(L))
    return inp


def weights(inp, zero_ambiguous):
    w = [inp[k].copy() for k in ("wf", "wc", "wn")]
    if zero_ambiguous:
        for x in w:
            x.reshape(3, -1)[:, inp["amb"]] = 0.0
    return w


def reference_run(inp, nv=None, texel_grads=True):
    """float64 reference_chain on the float32 inputs: forward planes and (full weights) per-pixel gradients; with texel_grads also the
    cubemap / fail gradients of the weights with the ambiguous pixels zeroed, and the texel-gradient scale S = sum_p |g_p|
    (the sum of |upstream at the lookup| over the footprints that touch each texel: the size of the terms each texel gradient sums)."""
    from helpers_chain import reference_chain
    from oracle import oracle as orc
    W, H = inp["W"], inp["H"]
    leaf = lambda x: torch.from_numpy(np.asarray(x, np.float32)).double().requires_grad_(True)
    nv_r = leaf(inp["nv"] if nv is None else nv)
    base_r, s_r, tex_r, fail_r = leaf(inp["base"]), leaf(inp["strength"]), leaf(inp["tex"]), leaf(inp["fail"])
    f, c, n = reference_chain(nv_r, base_r, s_r, tex_r, fail_r, inp["cam"], W, H)
    out = dict(final=f.detach().numpy(), refl=c.detach().numpy(), nworld=n.detach().numpy())
    loss = lambda w: (f * torch.from_numpy(w[0]).double()).sum() + (c * torch.from_numpy(w[1]).double()).sum() + (n * torch.from_numpy(w[2]).double()).sum()
    g = torch.autograd.grad(loss(weights(inp, False)), [nv_r, base_r, s_r], retain_graph=texel_grads)
    out.update(g_nv=g[0].numpy(), g_base=g[1].numpy(), g_s=g[2].numpy())
    if texel_grads:
        wz = weights(inp, True)
        gt = torch.autograd.grad(loss(wz), [tex_r, fail_r])
        out.update(g_tex=gt[0].numpy(), g_fail=gt[1].numpy())
        col = out["refl"].reshape(3, -1)
        g_look = np.abs((inp["strength"].reshape(1, -1) * wz[0].reshape(3, -1) + wz[1].reshape(3, -1)) * col * (1 - col))
        _, _, r = reference_dirs(nv_r.detach(), inp["cam"], W, H)
        # per texel, the sum of |upstream| over the footprints that touch it, bilinear weights replaced by 1: the oracle's backward at the
        # four corner texel centres of each footprint (weight 1 on that corner)
        face, lu, lv, _, _ = cube_coords(r.reshape(-1, 3).numpy(), inp["L"])
        x0, y0 = np.floor(lu - 0.5) + 0.5, np.floor(lv - 0.5) + 0.5
        tex64 = inp["tex"].astype(np.float64)
        out["tex_scale"] = sum(orc.cubemap_backward(np.ascontiguousarray(g_look), direction_of(face, x0 + i, y0 + j, inp["L"]), tex64, 1, 1,
                                                    dtype=np.float64)[1] for i in (0, 1) for j in (0, 1))
    return out


PATHS = ("forward_keys", "backward_keys", "atomics", "async_tail", "c_abi")


def hip_run(inp, path, zero_ambiguous):
    """One forward + backward of the two-node deferred reflection on cuda:0.  forward_keys / backward_keys: the sorted-footprint backward
    with the sort keys written by the forward / by the backward's pixel kernel; atomics: REFLECTION_BACKWARD_BINNED = False; async_tail:
    sorted footprints through a gradient sink with the tail on the side stream (small sort shape: no forward keys), joined by side_join;
    c_abi: the plain gsr_deferred_reflection_forward / _backward entry points (planar cubemap reads, no keys)."""
    import _gsr
    import gaussian_renderer as gr
    W, H, L = inp["W"], inp["H"], inp["L"]
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    cam = inp["cam"]
    ct = {k: cu(v) for k, v in cam.items() if isinstance(v, np.ndarray)}
    wf, wc, wn = (cu(w) for w in weights(inp, zero_ambiguous))
    if path == "c_abi":
        nv, base, s, tex, fail = cu(inp["nv"]), cu(inp["base"]), cu(inp["strength"]), cu(inp["tex"]), cu(inp["fail"])
        camb = gr._cam_block(ct["viewmatrix"], (H, W, cam["K"]), ct["R"], ct["T"])
        st = torch.cuda.current_stream().cuda_stream
        p = lambda t: t.data_ptr()
        final, col, nw = torch.empty_like(base), torch.empty_like(base), torch.empty_like(nv)
        assert _gsr.lib.gsr_deferred_reflection_forward(p(nv), p(base), p(s), p(camb), p(tex), p(fail), L, W, H, p(final), p(col), p(nw), st) == 0
        scratch = torch.empty(int(_gsr.lib.gsr_deferred_reflection_scratch_floats(L, W, H, 1)), dtype=torch.float32, device="cuda")
        g_nv, g_base, g_s = torch.empty_like(nv), torch.empty_like(base), torch.empty_like(s)
        g_tex, g_fail = torch.full_like(tex, float("nan")), torch.full_like(fail, float("nan"))
        assert _gsr.lib.gsr_deferred_reflection_backward(p(nv), p(base), p(s), p(camb), p(tex), p(fail), L, W, H, p(wf), p(wc), p(wn), p(g_nv),
                                                         p(g_base), p(g_s), p(g_tex), p(g_fail), p(scratch), scratch.numel(), st) == 0
        torch.cuda.synchronize()
        res = dict(final=final, refl=col, nworld=nw, g_nv=g_nv, g_base=g_base, g_s=g_s, g_tex=g_tex, g_fail=g_fail)
        return {k: v.cpu().numpy() for k, v in res.items()}
    saved = gr.REFLECTION_BACKWARD_BINNED, gr.REFLECTION_FORWARD_KEYS
    try:
        gr.REFLECTION_BACKWARD_BINNED = path != "atomics"
        gr.REFLECTION_FORWARD_KEYS = path == "forward_keys"
        leaf = lambda x: cu(x).requires_grad_(True)
        nv, base, s, tex, fail = leaf(inp["nv"]), leaf(inp["base"]), leaf(inp["strength"]), leaf(inp["tex"]), leaf(inp["fail"])

        class Env:
            params = {"Cubemap_texture": tex, "Cubemap_failv": fail}
        kw = {}
        if path == "async_tail":
            sink = {"cubemap": torch.full_like(tex, float("nan")), "fail": torch.full_like(fail, float("nan"))}
            kw = dict(grad_sink=sink, async_tail=True)
        f, c, n = gr.deferred_reflection(nv, base, s, Env(), ct["viewmatrix"], (H, W, cam["K"]), ct["R"], ct["T"], **kw)
        ((f * wf).sum() + (c * wc).sum() + (n * wn).sum()).backward()
        if path == "async_tail":
            assert tex.grad is None
            _gsr.side_join()
            g_tex, g_fail = sink["cubemap"], sink["fail"]
        else:
            g_tex, g_fail = tex.grad, fail.grad
        torch.cuda.synchronize()
        res = dict(final=f, refl=c, nworld=n, g_nv=nv.grad, g_base=base.grad, g_s=s.grad, g_tex=g_tex, g_fail=g_fail)
        return {k: v.detach().cpu().numpy() for k, v in res.items()}
    finally:
        gr.REFLECTION_BACKWARD_BINNED, gr.REFLECTION_FORWARD_KEYS = saved


def hip_outputs(inp, paths=PATHS):
    """{path: (outputs with full weights, outputs with the ambiguous pixels' weights zeroed)}."""
    return {p: (hip_run(inp, p, False), hip_run(inp, p, True)) for p in paths}


# ---- bars.  FWD_BAR: the suite's bar on the reflection's forward planes against float64 (tests/test_gpu_cubemap.py), 2e-5, scaled with L
# above 128 because the bilinear weights are differences of texel coordinates ~L/2 whose float32 resolution grows with L.
def fwd_bar(L):
    return 2e-5 * max(1.0, L / 128)


# Per-pixel gradients: |a - b| <= PX_RTOL |b| + px_floor(L) G, G the largest reference gradient among the pixels of the same |normal| decade
# (the normal gradient scales with 1 / (|n| + 1e-6): a tiny normal's must not set the floor of unit ones).  The texel coordinates
# of float32 and float64 differ by |dlu| < 2^-19 L (module docstring); the normal gradient is the bilinear slope (texel differences
# weighted by kx, ky) times the Jacobian of the lookup, so its error is |dlu| of that slope's size: px_floor = 2^-16 L = 8 |dlu|.
PX_RTOL = 1e-4


def px_floor(L):
    return max(2.0 ** -16 * L, 1e-5)


def _decades(inp):
    ln = np.linalg.norm(np.asarray(inp["nv"], np.float64).reshape(3, -1), axis=0)
    return np.where(ln > 0, np.floor(np.log10(np.maximum(ln, 1e-30))), -99).astype(int)


def pixel_gate(a, b, inp, sel, L):
    """Boolean [HW] of pixels in `sel` that fail the per-pixel gate (a, b: [C,H,W]), and the worst |a-b| / tol."""
    C = a.shape[0]
    a, b = a.reshape(C, -1).astype(np.float64), b.reshape(C, -1)
    tol = PX_RTOL * np.abs(b) + px_floor(L) * _decade_max(b, inp)[None]
    ratio = (np.abs(a - b) / np.maximum(tol, 1e-300)).max(axis=0)
    return (ratio > 1) & sel, float(ratio[sel].max()) if sel.any() else 0.0


# Texel gradients: a texel sums w_pk g_p over the footprints that reach it; the float32 weights differ from float64 by up to
# |dkx| + |dky| < 2^-18 L (module docstring) ABSOLUTE — a corner of small weight carries the same error as a large one — so
# |a - b| <= TEX_RTOL |b| + tex_floor(L) S, S = sum_p |g_p| over the footprints touching the texel (reference_run), tex_floor = 4x the bound.
TEX_RTOL = 1e-5


def tex_floor(L):
    return 2.0 ** -16 * L + 1e-6


def check_path(inp, ref, ref_env, got, name):
    """Every check of one path against the float64 reference: returns (observed worst ratios, 1 = at the bar; list of failures).
    ref_env: (lo, hi) envelopes of the pushed chains over the ambiguous pixels, for final / refl / nworld / g_nv / g_base / g_s."""
    L = inp["L"]
    full, zero = got
    amb = inp["amb"]
    ok = ~amb
    obs, fails = {}, []
    fb = fwd_bar(L)
    for k in ("final", "refl", "nworld"):
        d = np.abs(full[k].reshape(full[k].shape[0], -1) - ref[k].reshape(ref[k].shape[0], -1)).max(axis=0)
        obs[k] = float(d[ok].max()) / fb
        if (d[ok] > fb).any():
            fails.append((name, k, "pixels over the bar", int((d[ok] > fb).sum()), float(d[ok].max()), fb))
        if amb.any():
            lo, hi = ref_env[k]
            x = full[k].reshape(full[k].shape[0], -1)[:, amb]
            out = ((x < lo - fb) | (x > hi + fb)).any(axis=0)
            if out.any():
                fails.append((name, k, "ambiguous pixels outside the envelope", int(out.sum())))
    for k in ("g_nv", "g_base", "g_s"):
        bad, worst = pixel_gate(full[k], ref[k], inp, ok, L)
        obs[k] = worst
        if bad.any():
            kinds = np.bincount(inp["kind"][bad], minlength=len(KIND_NAMES))
            fails.append((name, k, "failing pixels by kind", {KIND_NAMES[i]: int(n) for i, n in enumerate(kinds) if n}, worst))
        if amb.any():
            out = outside_envelope(full[k], amb, ref_env[k], L, ref[k], inp)
            if out.any():
                kinds = np.bincount(inp["kind"][np.nonzero(amb)[0][out]], minlength=len(KIND_NAMES))
                fails.append((name, k, "ambiguous pixels outside the envelope", {KIND_NAMES[i]: int(n) for i, n in enumerate(kinds) if n}))
        # each pixel's gradient depends on its own upstream only: the run with the ambiguous pixels' weights zeroed agrees elsewhere
        C = full[k].shape[0]
        if not np.array_equal(zero[k].reshape(C, -1)[:, ok], full[k].reshape(C, -1)[:, ok]):
            fails.append((name, k, "per-pixel gradient depends on other pixels' weights"))
    for k, sk in (("g_tex", "tex_scale"), ("g_fail", None)):
        a, b = zero[k].astype(np.float64), ref[k]
        scale = ref[sk] if sk else np.abs(b)
        tol = TEX_RTOL * np.abs(b) + tex_floor(L) * scale + 1e-30
        r = np.abs(a - b) / tol
        obs[k] = float(r.max()) if np.isfinite(a).all() else float("inf")
        if not (r <= 1).all():
            fails.append((name, k, "elements over the bar", int((~(r <= 1)).sum()), obs[k]))
    return obs, fails


def _decade_max(b, inp):
    """[HW]: the largest |b| among the pixels of each pixel's |normal| decade (b: [C,H,W])."""
    b = np.abs(b.reshape(b.shape[0], -1)).max(axis=0)
    dec = _decades(inp)
    G = np.zeros(b.shape)
    for d in np.unique(dec):
        m = dec == d
        G[m] = b[m].max()
    return G


def outside_envelope(a, amb, env, L, ref, inp):
    """Boolean [n_ambiguous]: pixels whose per-pixel gradient a [C,H,W] leaves the envelope (lo, hi) by more than the per-pixel gate's bar
    of the unambiguous pixels: PX_RTOL of the envelope plus px_floor(L) times the largest reference gradient of the pixel's |normal| decade
    (ref [C,H,W]; a tiny normal's gradient, ~1e6 times larger, sets the floor of its own decade only)."""
    lo, hi = env
    x = a.reshape(a.shape[0], -1)[:, amb]
    slack = PX_RTOL * np.maximum(np.abs(lo), np.abs(hi)) + px_floor(L) * _decade_max(ref, inp)[amb][None]
    return ((x < lo - slack) | (x > hi + slack)).any(axis=0)


def random_inputs(nv, base, strength, tex, fail, wf, wc, wn, cam, L):
    """The `inp` dict of seam_inputs for a test's own inputs (numpy or CPU tensors), classified; kind is K_RANDOM everywhere."""
    a = lambda x: np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float32)
    H, W = a(nv).shape[1:]
    inp = dict(L=L, W=W, H=H, cam=cam, nv=a(nv), base=a(base), strength=a(strength), tex=a(tex), fail=a(fail), wf=a(wf), wc=a(wc),
               wn=a(wn), kind=np.full(W * H, K_RANDOM))
    cls, _, _, margin, _, _ = classify_image(inp["nv"], cam, W, H, L)
    inp.update(cls=cls, margin=margin, amb=margin < delta(L))
    return inp


def random_ambiguous_bound(L):
    """Expected ambiguous fraction of random directions: within DELTA of a border in either coordinate, 2 x 2 DELTA (borders one texel
    apart; the face ties add a fraction ~1/L of that), times 2 for room."""
    return 8 * delta(L)


def envelope(inp, ref):
    """(lo, hi) over the ambiguous pixels of the reference chain on the pushed normals (and the unpushed one)."""
    amb = np.nonzero(inp["amb"])[0]
    keys = [k for k in ("final", "refl", "nworld", "g_nv", "g_base", "g_s") if k in ref]
    vals = {k: [ref[k].reshape(ref[k].shape[0], -1)[:, amb]] for k in keys}
    for img in pushed_normals(inp["nv"], inp["cam"], inp["W"], inp["H"], inp["L"], amb):
        r = reference_run(inp, nv=img, texel_grads=False)
        for k in keys:
            vals[k].append(r[k].reshape(r[k].shape[0], -1)[:, amb])
    return {k: (np.min(v, axis=0), np.max(v, axis=0)) for k, v in vals.items()}


def child_dump(out_dir, sizes, paths=PATHS):
    """Entry point of the child process of the build-variant test: the HIP outputs of every path at each size, as out_dir/L<L>.npz."""
    os.makedirs(out_dir, exist_ok=True)
    for L in sizes:
        inp = seam_inputs(L, seed=L)
        arrays = {}
        for p in paths:
            full, zero = hip_run(inp, p, False), hip_run(inp, p, True)
            arrays.update({"%s/full/%s" % (p, k): v for k, v in full.items()})
            arrays.update({"%s/zero/%s" % (p, k): v for k, v in zero.items()})
        np.savez(os.path.join(out_dir, "L%d.npz" % L), **arrays)
    _, (full, zero) = mirror_case("vertex", 128, False)
    np.savez(os.path.join(out_dir, "mirror.npz"), **{"mirror/full/" + k: v for k, v in full.items()}, **{"mirror/zero/" + k: v for k, v in zero.items()})


def load_dump(path, paths=PATHS):
    z = np.load(path)
    return {p: tuple({k.split("/")[2]: z[k] for k in z.files if k.startswith(p + "/" + w + "/")} for w in ("full", "zero")) for p in paths}


def deviation(a, b, inp):
    """Largest difference of two HIP runs on the unambiguous pixels: forward planes absolute, per-pixel gradients relative to the largest
    reference-scale gradient of their |normal| decade, texel gradients relative to max |texel gradient|."""
    ok = ~inp["amb"]
    dev = {}
    for k in ("final", "refl", "nworld"):
        dev[k] = float(np.abs(a[0][k] - b[0][k]).reshape(3, -1)[:, ok].max())
    dec = _decades(inp)
    for k in ("g_nv", "g_base", "g_s"):
        C = a[0][k].shape[0]
        x, y = a[0][k].reshape(C, -1).astype(np.float64), b[0][k].reshape(C, -1)
        worst = 0.0
        for d in np.unique(dec[ok]):
            m = ok & (dec == d)
            worst = max(worst, float(np.abs(x[:, m] - y[:, m]).max() / max(np.abs(y[:, m]).max(), 1e-30)))
        dev[k] = worst
    dev["g_tex"] = float(np.abs(a[1]["g_tex"] - b[1]["g_tex"]).max() / max(np.abs(b[1]["g_tex"]).max(), 1e-30))
    return dev


# ---------------------------------------------------------------------------------------------- the fused node on a "mirror" scene
MIRROR_TARGETS = {"vertex": (1.0, 1.0, 1.0), "edge": (1.0, 1.0, 0.0)}     # cube vertex / midpoint of the edge between faces 0 and 2


def mirror_scene(target, L, W=SEAM_W, H=SEAM_H, seed=0):
    """One large, nearly opaque surfel filling a 2-degree view; its normal reflects the central view ray (+z) onto `target` (a cube vertex
    or an edge midpoint), so the reflected cone (~4.6 texels across at L = 128) is centred on it.  Returns (kw for rasterize_reflect as
    numpy arrays, cam, tex, fail)."""
    cam = S.make_camera(W, H, fovy_deg=2.0)
    v = np.asarray(MIRROR_TARGETS[target], np.float64)
    n = np.array([0.0, 0.0, 1.0]) - v / np.linalg.norm(v)
    n /= np.linalg.norm(n)
    axis = np.cross([0.0, 0.0, 1.0], n)
    ang = np.arccos(np.clip(n[2], -1, 1))
    q = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis / np.linalg.norm(axis)])     # (w, x, y, z): R e_z = n
    g = torch.Generator().manual_seed(seed)
    shs = torch.zeros(1, 16, 3)
    shs[0, 0] = torch.tensor([0.4, -0.2, 0.1])
    kw = dict(means3D=np.array([[0.0, 0.0, 3.0]], np.float32), opacities=np.array([[0.99]], np.float32), shs=shs.numpy(),
              refl_strengths=np.array([[0.7]], np.float32), scales=np.array([[0.8, 0.8]], np.float32), rotations=q[None].astype(np.float32),
              env_scope_mask=np.ones(1, bool))
    tex = (torch.rand(6, 3, L, L, generator=g) - 0.5).numpy()
    fail = (torch.randn(3, generator=g) * 0.5).numpy()
    return kw, cam, tex, fail


def mirror_run(kw, cam, tex, fail, weights_, async_tail):
    """rasterize_reflect forward + backward with upstream (wf, wc, wn) on (final, refl_color, normal_world); the texel gradients go to a
    sink (with async_tail: on the side stream, joined by side_join).  Returns (outputs and the pixel gradients the node's reflection backward
    handed its rasterizer backward, as numpy; normal_view = allmap[2:5], base colour and strength planes: the chain's inputs)."""
    import _gsr
    import gaussian_renderer as gr
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    W, H = int(cam["W"]), int(cam["H"])
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ct = {k: cu(v) for k, v in cam.items() if isinstance(v, np.ndarray)}
    st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.zeros(3, device="cuda"),
                                       scale_modifier=1.0, viewmatrix=ct["viewmatrix"], projmatrix=ct["projmatrix"], sh_degree=3,
                                       campos=ct["campos"], prefiltered=False, debug=False)
    t = {k: cu(v).requires_grad_(k != "env_scope_mask") for k, v in kw.items()}
    texc, failc = cu(tex).requires_grad_(True), cu(fail).requires_grad_(True)

    class Env:
        params = {"Cubemap_texture": texc, "Cubemap_failv": failc}
    sink = {"cubemap": torch.full_like(texc, float("nan")), "fail": torch.full_like(failc, float("nan"))}
    probe = {}
    gr._RasterizeReflect.probe = probe
    try:
        final, refl, nworld, base, _, allmap, refl_map, _ = gr.rasterize_reflect(
            GaussianRasterizer(st), Env(), ct["viewmatrix"], (H, W, cam["K"]), ct["R"], ct["T"], means3D=t["means3D"],
            means2D=torch.zeros_like(t["means3D"]).requires_grad_(True), opacities=t["opacities"], shs=t["shs"], refl_strengths=t["refl_strengths"],
            scales=t["scales"], rotations=t["rotations"], env_scope_mask=t["env_scope_mask"], refl_grad_sink=sink, async_tail=async_tail)
        wf, wc, wn = (cu(w.astype(np.float32)) for w in weights_)
        ((final * wf).sum() + (refl * wc).sum() + (nworld * wn).sum()).backward()
    finally:
        gr._RasterizeReflect.probe = None
    _gsr.side_join()
    torch.cuda.synchronize()
    npy = lambda x: x.detach().cpu().numpy()
    return dict(final=npy(final), refl=npy(refl), nworld=npy(nworld), nv=npy(allmap[2:5]), base=npy(base), strength=npy(refl_map),
                g_nv=npy(probe["g_normal_view"]), g_base=npy(probe["g_base"]), g_s=npy(probe["g_strength"]), g_tex=npy(sink["cubemap"]),
                g_fail=npy(sink["fail"]))


def mirror_case(target, L, async_tail, seed=0):
    """Both runs of the mirror scene (upstream everywhere; upstream zeroed on the ambiguous pixels, which the forward decides) and the
    `inp` of the float64 chain on the node's own planes.  Returns (inp, (full, zero))."""
    kw, cam, tex, fail = mirror_scene(target, L, seed=seed)
    W, H = int(cam["W"]), int(cam["H"])
    g = torch.Generator().manual_seed(7 + seed)
    w = [torch.randn(3, H, W, generator=g).numpy() for _ in range(3)]
    full = mirror_run(kw, cam, tex, fail, w, async_tail)
    inp = random_inputs(full["nv"], full["base"], full["strength"], tex, fail, w[0], w[1], w[2], cam, L)
    zero = mirror_run(kw, cam, tex, fail, weights(inp, True), async_tail)
    assert all(np.array_equal(zero[k], full[k]) for k in ("nv", "base", "strength"))
    return inp, (full, zero)
