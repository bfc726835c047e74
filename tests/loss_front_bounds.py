"""Float64 references with per-element error bounds for the loss front end (csrc/gsr_loss.hip): the photometric loss on the
composites of train.py:158-159 and the per-pixel gradient of the SSIM map, plus the seeded inputs their tests use.

References.  The composites v = rgb * alpha + (1 - alpha) * bg and g = gt * mask + (1 - mask) * bg are formed in float64 from
the float32 inputs; the float64 oracle (oracle/oracle_train.cpp, which accepts float64 images) gives the two sums and
dL/dv on them, and dL/drgb = alpha * dL/dv, dL/dalpha = sum_c (rgb - bg) * dL/dv are formed in numpy.  The map gradient is a
float64 restatement on loss_bounds.corr: the three derivative planes, then corr(G p0) + 2 x corr(G p1) + y corr(G p2).

Bounds.  The running-error scheme of loss_bounds._ssim_channel (same U, NCONV, NSUM and K = 2 per quantity), with inputs
that carry errors of their own.  A composite is four float32 operations:
    oma = 1 - a,  p1 = t * a,  p2 = oma * bg,  v = p1 + p2          (the last two may be one fused multiply-add)
and each contributes its magnitude (in units of u) unless its exact result is a float32 number, in which case it
contributes nothing: d_v = e(p1) + |bg| e(oma) + e(p2) + e(v), e(v) = |v| unless p1 or p2 is zero.  This covers the fused and
the unfused arrangement.  At alpha in {0, 1} (and wherever else every step is exact) d_v = 0: the composite is a float32 number
and any float32 evaluation gives it.  d_v and d_g then propagate through the five convolutions (corr of the input error, next
to the convolution's own NCONV roundings), the pointwise combination, the multiplication by alpha and the C-term sum.

The L1 term's gradient is sign(v - g).  Its float32 evaluation is the sign of the float64 one when |v - g| exceeds the
errors of both composites, or when both composites are exact (then an exact tie is a tie in float32 too: alpha = mask = 0
gives v = g = bg, alpha = mask = 1 with rgb == gt gives v = g = rgb).  `front_reference` asserts that one of the two holds at
every element: a seed that produces a near tie is replaced by another, no element is skipped."""
import numpy as np

import loss_bounds as LB
from loss_bounds import C1, C2, K_GRAD, K_SUM, NCONV, NSUM, U, corr

FRONT_SIZES = (1, 5, 6, 11, 27, 31, 32, 33, 37, 38, 43, 64, 65)
BACKGROUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.25, 0.6, 0.9))
COMBOS = ((True, True), (True, False), (False, True), (False, False))      # (alpha given, mask given)
ALPHA_KINDS = ("regions", "ramp", "noise", "outside")
MASK_KINDS = ("binary", "soft")


def front_shapes(seed, n):
    """n seeded (C, H, W) from FRONT_SIZES x FRONT_SIZES x {1, 2, 3, 5}, drawn as loss_bounds.ssim_shapes draws them."""
    rs = np.random.RandomState(seed)
    S = list(FRONT_SIZES)
    Hs = (S * (n // len(S) + 1))[:n]
    Ws = list(rs.permutation(S * (n // len(S) + 1))[:n])
    Cs = [(1, 2, 3, 5)[i % 4] for i in range(n)]
    return [(int(c), int(h), int(w)) for c, h, w in zip(Cs, Hs, Ws)]


def alpha_plane(kind, H, W, seed):
    """float32 [H, W].  regions: noise with bands of exact 0 and exact 1 that cross the 32-pixel tile edges (and each other);
    ramp: 0 .. 1 along the diagonal, inside (0, 1); noise; outside: values in [-0.3, 1.4] (the training loss does not clamp alpha)."""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    if kind == "regions":
        a = 0.05 + 0.9 * rs.rand(H, W)
        a[(ys % 32 >= 28) | (ys % 32 < 3)] = 0.0
        a[(xs % 32 >= 29) | (xs % 32 < 2)] = 1.0
        a[(ys + xs) % 19 < 3] = 0.0
    elif kind == "ramp":
        a = (ys + xs + rs.rand()) / (H + W - 1)          # (a seeded phase: another seed moves every value)
    elif kind == "noise":
        a = rs.rand(H, W)
    elif kind == "outside":
        a = -0.3 + 1.7 * rs.rand(H, W)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.float32)


def mask_plane(kind, H, W, seed):
    """float32 [H, W] in [0, 1]: binary (blobs of a thresholded low-pass noise, zero on the bands where alpha_plane("regions") is
    zero, so that v = g = bg there) or soft (the low-pass noise itself)."""
    rs = np.random.RandomState(seed + 7919)
    n = LB._lowpass(rs, (1, H, W))[0]
    if kind == "soft":
        return np.ascontiguousarray(n, np.float32)
    if kind != "binary":
        raise ValueError(kind)
    ys, xs = np.mgrid[0:H, 0:W]
    m = (n > 0.45).astype(np.float64)
    m[(ys % 32 >= 28) | (ys % 32 < 3)] = 0.0
    m[(xs % 32 >= 29) | (xs % 32 < 2)] = 1.0
    return np.ascontiguousarray(m, np.float32)


def front_case(family, shape, seed, combo=(True, True), alpha_kind="regions", mask_kind="binary", background=BACKGROUNDS[2]):
    """dict(rgb, gt [C, H, W]; alpha, mask [H, W] or None; bg [C]) float32: image content from loss_bounds.loss_pair.  A seed whose
    inputs hold a near tie of |v - g| (see near_ties) is replaced by seed + 1000, + 2000, ...: deterministic, and no element is skipped."""
    C, H, W = shape
    bg = np.array([background[c % 3] for c in range(C)], np.float32)
    for s in range(seed, seed + 20000, 1000):
        rgb, gt = LB.loss_pair(family, shape, s)
        case = dict(rgb=rgb, gt=gt, alpha=alpha_plane(alpha_kind, H, W, s) if combo[0] else None,
                    mask=mask_plane(mask_kind, H, W, s) if combo[1] else None, bg=bg, seed=s)
        if not near_ties(case).any():
            return case
    raise AssertionError(f"no seed without a near tie for {family} {shape} {seed}")


def _inexact(v):
    """1 where the float64 value is not a float32 number (a float32 operation with this exact result rounds), else 0."""
    with np.errstate(over="ignore"):
        return (v.astype(np.float32).astype(np.float64) != v).astype(np.float64)


def composite(t, a, bg):
    """(v, d_v): t * a + (1 - a) * bg in float64 from float32 inputs, and its float32 running error in units of u.
    t [C, H, W], a [H, W] or None (then v = t exactly), bg [C]."""
    t = np.asarray(t, np.float32).astype(np.float64)
    if a is None:
        return t, np.zeros(t.shape)
    a = np.asarray(a, np.float32).astype(np.float64)[None]
    b = np.asarray(bg, np.float32).astype(np.float64)[:, None, None]
    oma = 1.0 - a
    p1, p2 = t * a, oma * b            # (products of two float32 numbers: exact in float64)
    v = p1 + p2
    e_oma = np.abs(oma) * _inexact(oma)
    d_v = (np.abs(p1) * _inexact(p1) + np.abs(b) * e_oma + np.abs(p2) * _inexact(oma.astype(np.float32).astype(np.float64) * b)
           + np.abs(v) * ((p1 != 0) & (p2 != 0)))
    return v, d_v


def near_ties(case):
    """Boolean [C, H, W]: where the float32 sign of v - g is not defined by the float64 one: |v - g| within the rounding errors of
    the two composites and at least one of them inexact."""
    v, d_v = composite(case["rgb"], case["alpha"], case["bg"])
    g, d_g = composite(case["gt"], case["mask"], case["bg"])
    return (np.abs(v - g) <= K_GRAD * U * (d_v + d_g)) & ((d_v + d_g) > 0)


def channel(x, y, dx, dy):
    """loss_bounds._ssim_channel up to the derivative planes, on float64 planes x, y [H, W] that carry the input errors dx, dy
    (units of u).  Returns a dict: the map sv and its error, the planes p0, p1, p2 and theirs."""
    ax, ay = np.abs(x), np.abs(y)
    mu1, mu2 = corr(x), corr(y)
    e11, e22, e12 = corr(x * x), corr(y * y), corr(x * y)
    d_mu1, d_mu2 = NCONV * corr(ax) + corr(dx), NCONV * corr(ay) + corr(dy)
    d_e11, d_e22 = NCONV * e11 + corr(2 * ax * dx), NCONV * e22 + corr(2 * ay * dy)
    d_e12 = NCONV * corr(ax * ay) + corr(ax * dy + ay * dx)
    am1, am2 = np.abs(mu1), np.abs(mu2)
    mu1sq, mu2sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    d_mu1sq, d_mu2sq = 2 * am1 * d_mu1 + mu1sq, 2 * am2 * d_mu2 + mu2sq
    d_mu12 = am1 * d_mu2 + am2 * d_mu1 + np.abs(mu12)
    s1, s2, s12 = e11 - mu1sq, e22 - mu2sq, e12 - mu12
    d_s1, d_s2, d_s12 = d_e11 + d_mu1sq + np.abs(s1), d_e22 + d_mu2sq + np.abs(s2), d_e12 + d_mu12 + np.abs(s12)
    A, B = 2 * mu12 + C1, 2 * s12 + C2
    Cc, D = mu1sq + mu2sq + C1, s1 + s2 + C2
    d_A, d_B = 2 * d_mu12 + np.abs(A), 2 * d_s12 + np.abs(B)
    d_Cc, d_D = d_mu1sq + d_mu2sq + 2 * Cc, d_s1 + d_s2 + 2 * np.abs(D)
    aD = np.abs(D)
    P = Cc * D
    d_P = Cc * d_D + aD * d_Cc + np.abs(P)
    inv = 1.0 / P
    ainv = np.abs(inv)
    d_inv = d_P * ainv * ainv + ainv
    AB = A * B
    d_AB = np.abs(A) * d_B + np.abs(B) * d_A + np.abs(AB)
    sv = AB * inv
    asv = np.abs(sv)
    d_sv = ainv * d_AB + np.abs(AB) * d_inv + asv
    BA = B - A
    d_BA = d_A + d_B + np.abs(BA)
    m2ba = mu2 * BA
    d_m2ba = am2 * d_BA + np.abs(BA) * d_mu2 + np.abs(m2ba)
    t1 = 2 * m2ba * inv
    d_t1 = 2 * (ainv * d_m2ba + np.abs(m2ba) * d_inv) + np.abs(t1)
    DC = D - Cc
    d_DC = d_D + d_Cc + np.abs(DC)
    q1 = mu1 * sv
    d_q1 = am1 * d_sv + asv * d_mu1 + np.abs(q1)
    q2 = q1 * DC
    d_q2 = np.abs(q1) * d_DC + np.abs(DC) * d_q1 + np.abs(q2)
    t2 = 2 * q2 * inv
    d_t2 = 2 * (ainv * d_q2 + np.abs(q2) * d_inv) + np.abs(t2)
    p0 = t1 - t2
    p1 = -sv / D
    p2 = 2 * A * inv
    return dict(sv=sv, d_sv=d_sv, p=(p0, p1, p2),
                d_p=(d_t1 + d_t2 + np.abs(p0), d_sv / aD + asv * d_D / (aD * aD) + np.abs(p1), 2 * (ainv * d_A + np.abs(A) * d_inv) + np.abs(p2)))


def adjoint(planes, d_planes, x, y, dx, dy):
    """(t, d_t): t = corr(q0) + 2 x corr(q1) + y corr(q2) on planes q with errors d_q, at pixels x, y with errors dx, dy."""
    c = [corr(q) for q in planes]
    d_c = [corr(dq) + NCONV * corr(np.abs(q)) for q, dq in zip(planes, d_planes)]
    ax, ay = np.abs(x), np.abs(y)
    xc1, yc2 = 2 * x * c[1], y * c[2]
    s01 = c[0] + xc1
    t = s01 + yc2
    d_t = (d_c[0] + 2 * ax * d_c[1] + 2 * np.abs(c[1]) * dx + np.abs(xc1) + ay * d_c[2] + np.abs(c[2]) * dy + np.abs(yc2)
           + np.abs(s01) + np.abs(t))
    return t, d_t


def front_reference(case, w_l1, w_ssim):
    """Float64 oracle values and bounds of gsr_photometric_forward / _backward on a front_case with float32 weights.
    Returns ref and bnd dicts with l1, ssim (the sums), dv [C, H, W] (dL/dv), drgb [C, H, W] and, with alpha, dalpha [H, W]."""
    from oracle import oracle as orc
    rgb32, bg32 = case["rgb"], case["bg"]
    w_l1, w_ssim = float(np.float32(w_l1)), float(np.float32(w_ssim))
    v, d_v = composite(rgb32, case["alpha"], bg32)
    g, d_g = composite(case["gt"], case["mask"], bg32)
    near = near_ties(case)
    assert not near.any(), f"{int(near.sum())} near ties of |v - g| (first at {np.argwhere(near)[0].tolist()}): choose another seed"
    s_l1, s_ss, _ = orc.ssim_l1_forward(v, g, C1, C2, dtype=np.float64)
    dv = orc.ssim_l1_backward(v, g, w_l1, w_ssim, C1, C2, dtype=np.float64)
    C = v.shape[0]
    b_dv = np.empty(v.shape)
    k_l1 = k_ss = 0.0
    for c in range(C):
        ch = channel(v[c], g[c], d_v[c], d_g[c])
        t, d_t = adjoint(ch["p"], ch["d_p"], v[c], g[c], d_v[c], d_g[c])
        gr = w_l1 * np.sign(v[c] - g[c]) + w_ssim * t
        b_dv[c] = abs(w_ssim) * d_t + np.abs(w_ssim * t) + np.abs(gr)
        k_l1 += (d_v[c] + d_g[c]).sum() + (NSUM + 1) * np.abs(v[c] - g[c]).sum()
        k_ss += ch["d_sv"].sum() + NSUM * np.abs(ch["sv"]).sum()
    ref = dict(l1=s_l1, ssim=s_ss, dv=dv)
    bnd = dict(l1=K_SUM * U * (k_l1 + abs(s_l1)), ssim=K_SUM * U * (k_ss + abs(s_ss)), dv=K_GRAD * U * b_dv)
    if case["alpha"] is None:
        ref["drgb"], bnd["drgb"] = dv, bnd["dv"]
    else:
        a = case["alpha"].astype(np.float64)[None]
        ref["drgb"] = a * dv
        bnd["drgb"] = K_GRAD * U * (np.abs(a) * b_dv + np.abs(ref["drgb"]))
        diff = rgb32.astype(np.float64) - bg32.astype(np.float64)[:, None, None]
        prod = diff * dv
        ref["dalpha"] = prod.sum(0)
        # per term: the difference's rounding and the product's (2 |prod|) next to dL/dv's own error; then C additions, each
        # rounding a partial sum that is at most sum |prod|
        bnd["dalpha"] = K_GRAD * U * ((np.abs(diff) * b_dv + 2 * np.abs(prod)).sum(0) + C * np.abs(prod).sum(0))
    return ref, bnd


def map_grad_reference(img1, img2, G):
    """Float64 reference and bound of gsr_ssim_map_backward on float32 images [P, H, W] and a float32 upstream gradient G
    [P, H, W]: corr(G p0) + 2 x corr(G p1) + y corr(G p2), the planes as loss_bounds._ssim_channel forms them.  The kernel reads the
    float32 planes a forward left (their errors d_p), multiplies by G (one rounding) and convolves."""
    x32, y32, G32 = (np.ascontiguousarray(t, np.float32) for t in (img1, img2, G))
    ref, bnd = np.empty(x32.shape, np.float64), np.empty(x32.shape, np.float64)
    zero = np.zeros(x32.shape[1:])
    for c in range(x32.shape[0]):
        x, y, Gc = x32[c].astype(np.float64), y32[c].astype(np.float64), G32[c].astype(np.float64)
        ch = channel(x, y, zero, zero)
        q = [Gc * p for p in ch["p"]]
        d_q = [np.abs(Gc) * dp + np.abs(qq) for qq, dp in zip(q, ch["d_p"])]
        t, d_t = adjoint(q, d_q, x, y, zero, zero)
        ref[c], bnd[c] = t, K_GRAD * U * d_t
    return ref, bnd


def chain_f32(case, w_l1, w_ssim):
    """The whole chain in float32 on the CPU (numpy composites, the float32 oracle, numpy products): a second float32
    implementation for the bounds to hold."""
    from oracle import oracle as orc
    f = np.float32
    rgb, gt, bg = case["rgb"], case["gt"], case["bg"][:, None, None]
    one = f(1.0)
    v = rgb if case["alpha"] is None else rgb * case["alpha"][None] + (one - case["alpha"][None]) * bg
    g = gt if case["mask"] is None else gt * case["mask"][None] + (one - case["mask"][None]) * bg
    v, g = np.ascontiguousarray(v, f), np.ascontiguousarray(g, f)
    l1, ss, _ = orc.ssim_l1_forward(v, g, C1, C2, dtype=f)
    dv = orc.ssim_l1_backward(v, g, f(w_l1), f(w_ssim), C1, C2, dtype=f)
    out = dict(l1=l1, ssim=ss, dv=dv, drgb=dv)
    if case["alpha"] is not None:
        out["drgb"] = case["alpha"][None] * dv
        acc = np.zeros(dv.shape[1:], f)
        for c in range(dv.shape[0]):
            acc = acc + (rgb[c] - bg[c]) * dv[c]
        out["dalpha"] = acc
    return out


def check_front(got, ref, bnd, what):
    """Every output present in `got` within its bound (loss_bounds.check: no budget of failing elements)."""
    worst = {}
    for k in ("l1", "ssim", "dv", "drgb", "dalpha"):
        if k in got and got[k] is not None:
            worst[k] = LB.check(got[k], ref[k], bnd[k], what=f"{what} {k}")
    return worst
