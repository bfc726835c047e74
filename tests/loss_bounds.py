"""Float64 references with per-element error bounds for the training-step kernels around the rasterizer: the fused SSIM + L1
loss, the surface pass and the flat Adam step (csrc/gsr_loss.hip, csrc/gsr_surface.hip, csrc/gsr_train.hip), plus the seeded inputs their
tests use.

The reference value of each output comes from the float64 oracle (oracle/oracle_train.cpp), evaluated on the same float32
inputs and float32 constants the kernels receive.  Beside it this module computes, in float64 from the same inputs, a bound
on how far ANY float32 evaluation of the same expression may land from it:

    |fp32 result - float64 reference| <= K * u * kappa,       u = 2**-24

kappa is the running-error estimate of the expression: every intermediate is replaced by its magnitude, each operation adds
its own rounding (|result|, in units of u) to the propagated errors of its operands, and divisions, square roots and
products propagate first order (d(a/b) = da/|b| + |a| db / b^2).  A convolution with the 11 x 11 window counts as NCONV
roundings of the convolution of the magnitudes, the worst case of the kernel's separable 11 + 11 sums.  K (one per quantity) absorbs the second-order terms that first-order propagation drops and the
differences in how the kernel and the oracle arrange the same expression; it is fixed, not fitted per case.

Where an input is non-finite the outputs that depend on it are compared by class instead (NaN with NaN, an infinity with an
infinity of the same sign), see `check`.
"""
import numpy as np

U = 2.0 ** -24
F32_MAX = float(np.finfo(np.float32).max)

# ------------------------------------------------------------------------------------------------------------- SSIM + L1
C1 = float(np.float32(0.01 ** 2))        # the constants the kernels receive (float32), given to the float64 oracle as well
C2 = float(np.float32(0.03 ** 2))
# A convolution is bounded as the kernel evaluates it: two separable passes of 11 products and sums (22 roundings of the
# convolution of the magnitudes), +1 for the window's float32 outer product g_i g_j, +1 for the squared or mixed input.  The
# oracle's 121-term sequential sum has a larger worst case (121) but lands far inside this one in practice: its errors are
# those of a sum of same-signed terms, growing like a random walk, and test_loss_bounds checks it at every element.
NCONV = 24
NSUM = 16          # additions a pixel's term passes through in the kernel's block reduction (4 rows + 6 wave + 3 block levels)
K_MAP = 2.0        # SSIM map
K_SUM = 2.0        # both sums
K_GRAD = 2.0       # image gradient


def window1d():
    """The reference's 1-D window as the kernels build it: float32 exp values normalised by their float32 sum."""
    g = np.array([np.float32(np.exp(-((i - 5) ** 2) / (2.0 * 1.5 * 1.5))) for i in range(11)], np.float32)
    return (g / g.sum(dtype=np.float32)).astype(np.float64)


_G = window1d()


def corr(p):
    """Zero-padded 11 x 11 correlation of a float64 plane [H, W] with the separable window (magnitudes only: the separable
    window differs from the oracle's float32 outer product by at most one rounding per weight)."""
    H, W = p.shape
    q = np.zeros((H, W + 10))
    q[:, 5:5 + W] = p
    h = _G[0] * q[:, 0:W]
    for k in range(1, 11):
        h += _G[k] * q[:, k:k + W]
    q = np.zeros((H + 10, W))
    q[5:5 + H] = h
    out = _G[0] * q[0:H]
    for k in range(1, 11):
        out += _G[k] * q[k:k + H]
    return out


def _ssim_channel(x, y, w_l1, w_ssim):
    """Running-error estimates (units of u) of one channel: map, |map|, |x - y| and the image gradient."""
    ax, ay = np.abs(x), np.abs(y)
    mu1, mu2 = corr(x), corr(y)
    e11, e22, e12 = corr(x * x), corr(y * y), corr(x * y)
    d_mu1, d_mu2 = NCONV * corr(ax), NCONV * corr(ay)
    d_e11, d_e22, d_e12 = NCONV * e11, NCONV * e22, NCONV * corr(ax * ay)
    am1, am2 = np.abs(mu1), np.abs(mu2)
    mu1sq, mu2sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    d_mu1sq, d_mu2sq = 2 * am1 * d_mu1 + mu1sq, 2 * am2 * d_mu2 + mu2sq
    d_mu12 = am1 * d_mu2 + am2 * d_mu1 + np.abs(mu12)
    s1, s2, s12 = e11 - mu1sq, e22 - mu2sq, e12 - mu12
    d_s1, d_s2, d_s12 = d_e11 + d_mu1sq + np.abs(s1), d_e22 + d_mu2sq + np.abs(s2), d_e12 + d_mu12 + np.abs(s12)
    A, B = 2 * mu12 + C1, 2 * s12 + C2
    Cc, D = mu1sq + mu2sq + C1, s1 + s2 + C2          # Cc >= C1 and D >= C2 (a windowed variance is >= 0): all finite
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
    # the three derivative planes, in the kernel's arrangement
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
    d_p0 = d_t1 + d_t2 + np.abs(p0)
    p1 = -sv / D
    d_p1 = d_sv / aD + asv * d_D / (aD * aD) + np.abs(p1)
    p2 = 2 * A * inv
    d_p2 = 2 * (ainv * d_A + np.abs(A) * d_inv) + np.abs(p2)
    # adjoint convolutions (input errors of the planes + the convolution's own) and the pointwise combination
    c0, c1, c2 = corr(p0), corr(p1), corr(p2)
    d_c0 = corr(d_p0) + NCONV * corr(np.abs(p0))
    d_c1 = corr(d_p1) + NCONV * corr(np.abs(p1))
    d_c2 = corr(d_p2) + NCONV * corr(np.abs(p2))
    xc1, yc2 = 2 * x * c1, y * c2
    s01 = c0 + xc1
    t = s01 + yc2
    d_t = d_c0 + 2 * ax * d_c1 + np.abs(xc1) + ay * d_c2 + np.abs(yc2) + np.abs(s01) + np.abs(t)
    g = w_l1 * np.sign(x - y) + w_ssim * t
    d_g = abs(w_ssim) * d_t + np.abs(w_ssim * t) + np.abs(g)
    return d_sv, asv, np.abs(x - y), d_g


def ssim_reference(img1, img2, w_l1, w_ssim):
    """Float64 oracle values and error bounds of the fused loss on float32 images [C, H, W] with float32 weights.
    Returns dict(l1, ssim, map, grad) of references and dict(l1, ssim, map, grad) of bounds."""
    from oracle import oracle as orc
    x32, y32 = np.ascontiguousarray(img1, np.float32), np.ascontiguousarray(img2, np.float32)
    w_l1, w_ssim = float(np.float32(w_l1)), float(np.float32(w_ssim))
    s_l1, s_ss, smap = orc.ssim_l1_forward(x32, y32, C1, C2, dtype=np.float64)
    grad = orc.ssim_l1_backward(x32, y32, w_l1, w_ssim, C1, C2, dtype=np.float64)
    C = x32.shape[0]
    b_map, b_grad = np.empty(smap.shape), np.empty(smap.shape)
    k_l1 = k_ss = 0.0
    for c in range(C):
        d_sv, asv, al1, d_g = _ssim_channel(x32[c].astype(np.float64), y32[c].astype(np.float64), w_l1, w_ssim)
        b_map[c] = K_MAP * U * d_sv
        b_grad[c] = K_GRAD * U * d_g
        k_l1 += (NSUM + 1) * al1.sum()
        k_ss += d_sv.sum() + NSUM * asv.sum()
    ref = dict(l1=s_l1, ssim=s_ss, map=smap, grad=grad)
    bnd = dict(l1=K_SUM * U * (k_l1 + abs(s_l1)), ssim=K_SUM * U * (k_ss + abs(s_ss)), map=b_map, grad=b_grad)
    return ref, bnd


# ------------------------------------------------------------------------------------------------------------- surface pass
ALPHA_MIN = float(np.float32(1e-3))       # the kernels' clamp(alpha, 1e-3) and normalize eps, as float32 values
NORM_EPS = float(np.float32(1e-12))
K_SD = 2.0          # surf_depth
K_N = 2.0           # surf_normal
K_GALL = 4.0        # g_allmap: the kernel gathers what the oracle scatters (each point's four terms in another order)
POISON = 1e9        # |point| beyond which |cross product|^2 may overflow float32: not defined by a float64 reference


def _nan_to_num00(v):
    out = np.where(np.isnan(v) | (v == np.inf), 0.0, v)
    return np.where(out == -np.inf, -F32_MAX, out)


def _shift(a, dy, dx):
    """out[y, x] = a[y + dy, x + dx] (zero outside), on the last two axes."""
    out = np.zeros_like(a)
    H, W = a.shape[-2], a.shape[-1]
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def _dilate(mask, r):
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out |= _shift(mask, dy, dx)
    return out


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _d_cross(a, b, da, db, c):
    """Running error of c = a x b (component-wise, units of u)."""
    A, B = np.abs(a), np.abs(b)
    out = []
    for i, j in ((1, 2), (2, 0), (0, 1)):
        out.append(A[i] * db[j] + B[j] * da[i] + A[i] * B[j] + A[j] * db[i] + B[i] * da[j] + A[j] * B[i])
    return np.stack(out) + np.abs(c)


def surface_reference(allmap, raymat, depth_ratio, g_surf_depth=None, g_surf_normal=None):
    """Float64 oracle values and bounds of the surface pass on a float32 allmap [8, H, W] and raymat [12].
    Returns (ref, bnd, skip): ref/bnd dicts with sd [H, W], sn [3, H, W] and, when a cotangent is given, g [8, H, W]; skip is
    the dict of boolean masks of elements the float64 reference does not define (an intermediate beyond the float32 range,
    or a cross product within rounding of the normalize eps, where the kernel may take either branch)."""
    from oracle import oracle as orc
    am = np.ascontiguousarray(allmap, np.float32)
    ray32 = np.ascontiguousarray(raymat, np.float32).reshape(12)
    r = float(np.float32(depth_ratio))
    gsd32 = None if g_surf_depth is None else np.ascontiguousarray(g_surf_depth, np.float32).reshape(am.shape[1:])
    gsn32 = None if g_surf_normal is None else np.ascontiguousarray(g_surf_normal, np.float32)
    sd, sn, gam = orc.surface_pass(am, ray32, r, gsd32, gsn32, dtype=np.float64, fp32_constants=True)
    H, W = am.shape[1], am.shape[2]
    a64 = am.astype(np.float64)
    M = ray32.astype(np.float64)
    D, A, med = a64[0], a64[1], a64[5]
    with np.errstate(all="ignore"):
        cl = np.maximum(A, ALPHA_MIN)
        e = D / cl
        fin_e = np.isfinite(e)
        e0 = _nan_to_num00(e)
        m0 = _nan_to_num00(med)
        d_e = np.abs(e0)
        ome = 1.0 - r
        d_ome = abs(ome)
        t1, t2 = e0 * ome, r * m0
        sdv = t1 + t2
        d_sd = abs(ome) * d_e + np.abs(e0) * d_ome + np.abs(t1) + np.abs(t2) + np.abs(sdv)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        rd = np.stack([xs * M[j] + ys * M[3 + j] + M[6 + j] for j in range(3)])
        d_rd = np.stack([2 * np.abs(xs * M[j]) + np.abs(ys * M[3 + j]) + np.abs(xs * M[j] + ys * M[3 + j]) + np.abs(rd[j]) for j in range(3)])
        P = sdv * rd + M[9:12, None, None]
        d_P = np.abs(rd) * d_sd + np.abs(sdv) * d_rd + np.abs(sdv * rd) + np.abs(P)
        big = (np.abs(P) > POISON).any(0) | ~np.isfinite(P).all(0)
        a = _shift(P, 1, 0) - _shift(P, -1, 0)
        b = _shift(P, 0, 1) - _shift(P, 0, -1)
        d_a = _shift(d_P, 1, 0) + _shift(d_P, -1, 0) + np.abs(a)
        d_b = _shift(d_P, 0, 1) + _shift(d_P, 0, -1) + np.abs(b)
        c = _cross(a, b)
        d_c = _d_cross(a, b, d_a, d_b, c)
        s = (c * c).sum(0)
        ln = np.sqrt(s)
        d_s = (2 * np.abs(c) * d_c + c * c).sum(0) + 2 * s
        d_len = np.where(ln > 0, d_s / (2 * np.where(ln > 0, ln, 1.0)), np.sqrt(d_s)) + ln
        den = np.maximum(ln, NORM_EPS)
        inv = 1.0 / den
        d_inv = d_len * inv * inv + inv
        aA = np.abs(A)
        d_n = aA[None] * (inv * d_c + np.abs(c) * d_inv + np.abs(c) * inv) + np.abs(c * inv * A)
    interior = np.zeros((H, W), bool)
    interior[1:H - 1, 1:W - 1] = True
    # surf_normal reads the points at its four neighbours; a stencil touching a point beyond the float32 range is undefined here
    sn_skip = interior & (_shift(big, 1, 0) | _shift(big, -1, 0) | _shift(big, 0, 1) | _shift(big, 0, -1))
    ambiguous = interior & (np.abs(ln - NORM_EPS) <= K_N * U * d_len)
    ref = dict(sd=sd, sn=sn)
    bnd = dict(sd=K_SD * U * d_sd, sn=np.where(interior[None], K_N * U * d_n, 0.0))
    skip = dict(sd=np.zeros((H, W), bool), sn=np.broadcast_to(sn_skip, (3, H, W)))
    if gam is None:
        return ref, bnd, skip
    with np.errstate(all="ignore"):
        gsd = np.zeros((H, W)) if gsd32 is None else gsd32.astype(np.float64)
        gsn = np.zeros((3, H, W)) if gsn32 is None else gsn32.astype(np.float64)
        gn = gsn * A[None]
        d_gn = np.abs(gn)
        big_branch = ln > NORM_EPS
        lnz = np.where(big_branch, ln, 1.0)
        n = c / lnz
        d_nn = d_c / lnz + np.abs(c) * d_len / (lnz * lnz) + np.abs(n)
        dd = (n * gn).sum(0)
        d_dd = (np.abs(gn) * d_nn + np.abs(n) * d_gn + 3 * np.abs(n * gn)).sum(0)
        num = gn - n * dd
        d_num = d_gn + np.abs(dd) * d_nn + np.abs(n) * d_dd + np.abs(n * dd) + np.abs(num)
        gc_hi = num / lnz
        d_gc_hi = d_num / lnz + np.abs(num) * d_len / (lnz * lnz) + np.abs(gc_hi)
        gc_lo = gn / NORM_EPS
        d_gc_lo = d_gn / NORM_EPS + 2 * np.abs(gc_lo)
        gc = np.where(big_branch, gc_hi, gc_lo)
        d_gc = np.where(big_branch, d_gc_hi, d_gc_lo)
        gc = np.where(interior, gc, 0.0)
        d_gc = np.where(interior, d_gc, 0.0)
        ga, gb = _cross(b, gc), _cross(gc, a)
        d_ga, d_gb = _d_cross(b, gc, d_b, d_gc, ga), _d_cross(gc, a, d_gc, d_a, gb)
        terms = [_shift(ga, -1, 0), _shift(ga, 1, 0), _shift(gb, 0, -1), _shift(gb, 0, 1)]
        gP = terms[0] - terms[1] + terms[2] - terms[3]
        d_gP = (_shift(d_ga, -1, 0) + _shift(d_ga, 1, 0) + _shift(d_gb, 0, -1) + _shift(d_gb, 0, 1)
                + 3 * sum(np.abs(t) for t in terms))
        prod = gP * rd
        g_s = prod.sum(0) + gsd
        d_gs = (np.abs(rd) * d_gP + np.abs(gP) * d_rd + 3 * np.abs(prod)).sum(0) + np.abs(g_s)
        ge = np.where(fin_e, g_s * ome, 0.0)
        d_ge = np.where(fin_e, abs(ome) * d_gs + np.abs(g_s) * d_ome + np.abs(ge), 0.0)
        b0 = d_ge / cl + np.abs(ge / cl)
        b1 = np.where(A >= ALPHA_MIN, (np.abs(D) * d_ge + 3 * np.abs(ge * D)) / (cl * cl), 0.0)
        b5 = np.where(np.isfinite(med), abs(r) * d_gs + np.abs(g_s * r), 0.0)
    bg = np.zeros((8, H, W))
    bg[0], bg[1], bg[5] = K_GALL * U * b0, K_GALL * U * b1, K_GALL * U * b5
    # the gradient at q gathers the cross products at q +- 1, each of which reads points at +- 1 of it
    g_skip = _dilate(sn_skip | ambiguous, 1) | _dilate(big, 2)
    ref["g"], bnd["g"] = gam, bg
    skip["g"] = np.broadcast_to(g_skip, (8, H, W))
    return ref, bnd, skip


# ------------------------------------------------------------------------------------------------------------------- Adam
K_ADAM = 2.0


def adam_reference(p, g, m, v, lr, beta1, beta2, eps, step):
    """Float64 oracle step of torch.optim.Adam on float32 state with float32 hyper-parameters and per-element learning rates.
    Returns ((p, m, v) references, (p, m, v) bounds)."""
    from oracle import oracle as orc
    f = lambda t: float(np.float32(t))
    b1, b2, ep = f(beta1), f(beta2), f(eps)
    arrs = [np.ascontiguousarray(t, np.float32).reshape(-1).astype(np.float64) for t in (p, g, m, v, lr)]
    p64, g64, m64, v64, lr64 = arrs
    rp, rm, rv = orc.adam(p64, g64, m64, v64, lr64, beta1=b1, beta2=b2, eps=ep, step=int(step), dtype=np.float64)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    sq = np.sqrt(bc2)
    with np.errstate(all="ignore"):
        d_m = np.abs(b1 * m64) + 2 * np.abs((1 - b1) * g64) + np.abs(rm)
        gg = g64 * g64
        d_v = np.abs(b2 * v64) + 3 * np.abs((1 - b2) * gg) + np.abs(rv)
        s = np.sqrt(rv)
        d_s = np.where(s > 0, d_v / (2 * np.where(s > 0, s, 1.0)), 0.0) + s
        q = s / sq
        d_q = d_s / sq + 2 * q
        den = q + ep
        d_den = d_q + den
        rr = rm / den
        d_r = d_m / den + np.abs(rm) * d_den / (den * den) + np.abs(rr)
        st = lr64 / bc1
        upd = st * rr
        d_upd = np.abs(st) * d_r + 2 * np.abs(upd) + np.abs(upd)
        d_p = d_upd + np.abs(rp)
    return (rp, rm, rv), (K_ADAM * U * d_p, K_ADAM * U * d_m, K_ADAM * U * d_v)


# ------------------------------------------------------------------------------------------------------------- comparison
def check(got, ref, bound, skip=None, what=""):
    """Per element: finite references within the bound, non-finite references by class.  No budget of failing elements.
    Returns the largest |got - ref| / bound over the compared elements."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    use = np.ones(ref.shape, bool) if skip is None else ~np.asarray(skip)
    fin = np.isfinite(ref) & use
    nan = np.isnan(ref) & use
    inf = np.isinf(ref) & use
    assert np.isnan(got[nan]).all(), f"{what}: NaN expected at {np.argwhere(nan & ~np.isnan(got))[:5].tolist()}"
    assert (got[inf] == ref[inf]).all(), f"{what}: infinity expected at {np.argwhere(inf & (got != ref))[:5].tolist()}"
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    bad = fin & ~(err <= bound)
    if bad.any():
        idx = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(fin.sum())} elements outside the bound; first at {list(idx)}: "
                             f"got {got[idx]!r}, ref {ref[idx]!r}, bound {bound[idx]!r}")
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(fin & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    return float(q.max()) if q.size else 0.0


# ---------------------------------------------------------------------------------------------------- seeded loss inputs
SSIM_SIZES = (1, 2, 5, 6, 10, 11, 21, 26, 27, 31, 32, 33, 37, 38, 42, 43, 63, 64, 65)   # tile and halo edges at every offset
STEP_OFFSETS = (0, 4, 5, 6, 26, 27, 31)                                                   # step edges, mod the 32-pixel tile
FAMILIES = ("uniform", "lowpass", "bright_flat", "constant_pair", "identical", "ties", "checker", "hdr", "zeros", "steps")


def _lowpass(rs, shape):
    C, H, W = shape
    n = rs.rand(C, H + 8, W + 8)
    k = np.ones(9) / 9.0
    n = np.apply_along_axis(lambda r: np.convolve(r, k, "valid"), 2, n)
    n = np.apply_along_axis(lambda r: np.convolve(r, k, "valid"), 1, n)
    return (n - n.min()) / max(n.max() - n.min(), 1e-12)


def _steps(shape, phase):
    C, H, W = shape
    ys, xs = np.arange(H), np.arange(W)
    sy = np.isin((ys + phase) % 32, STEP_OFFSETS).cumsum() % 2
    sx = np.isin((xs + 2 * phase) % 32, STEP_OFFSETS).cumsum() % 2
    return np.broadcast_to(0.2 + 0.5 * sy[:, None] + 0.25 * sx[None, :], shape)


def loss_pair(family, shape, seed):
    """(img1, img2) float32 [C, H, W] of a content family; img1 is the rendered image (gets the gradient), img2 the target."""
    rs = np.random.RandomState(seed)
    C, H, W = shape
    if family == "uniform":
        y = rs.rand(C, H, W)
        x = 0.6 * y + 0.4 * rs.rand(C, H, W)
    elif family == "lowpass":
        y = _lowpass(rs, shape)
        x = np.clip(y + 0.05 * (_lowpass(rs, shape) - 0.5), 0, 1)
    elif family == "bright_flat":          # E[x^2] - mu^2 cancels: D is within a few C2 of C2
        y = 0.9 + 1e-3 * (2 * rs.rand(C, H, W) - 1)
        x = 0.9 + 1e-3 * (2 * rs.rand(C, H, W) - 1)
    elif family == "constant_pair":
        x, y = np.full(shape, 0.3), np.full(shape, 0.7)
    elif family == "identical":
        y = rs.rand(C, H, W)
        x = y.copy()
    elif family == "ties":                 # half the pixels exactly tied: the L1 gradient there is sign(0) = 0
        y = rs.rand(C, H, W).astype(np.float32)
        x = np.where(rs.rand(C, H, W) < 0.5, y, rs.rand(C, H, W).astype(np.float32))
    elif family == "checker":              # period 2: the largest possible local variance
        cb = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.float64)
        x = np.broadcast_to(cb, shape).copy()
        y = np.broadcast_to(0.25 + 0.5 * (1 - cb), shape).copy()
    elif family == "hdr":                  # renders are not clamped: values outside [0, 1]
        y = -0.5 + 4.5 * rs.rand(C, H, W)
        x = -0.5 + 4.5 * rs.rand(C, H, W)
    elif family == "zeros":
        x, y = np.zeros(shape), np.zeros(shape)
    elif family == "steps":
        x = _steps(shape, 0) + 0.02 * rs.rand(C, H, W)
        y = _steps(shape, 1)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


def ssim_shapes(seed, n):
    """n seeded (C, H, W) from SSIM_SIZES x SSIM_SIZES x {1, 2, 3, 5}; every size appears as H and as W."""
    rs = np.random.RandomState(seed)
    S = list(SSIM_SIZES)
    Hs = (S * (n // len(S) + 1))[:n]
    Ws = list(rs.permutation(S * (n // len(S) + 1))[:n])
    Cs = [(1, 2, 3, 5)[i % 4] for i in range(n)]
    return [(int(c), int(h), int(w)) for c, h, w in zip(Cs, Hs, Ws)]


# ------------------------------------------------------------------------------------------------- seeded surface inputs
SURF_SIZES = (1, 2, 3, 4, 15, 16, 17, 18, 31, 32, 33, 34)     # 16-pixel tile, halo 1 forward / 2 backward
ALPHA_CASES = (0.0, float(np.nextafter(np.float32(ALPHA_MIN), np.float32(0))), ALPHA_MIN,
               float(np.nextafter(np.float32(ALPHA_MIN), np.float32(1))))


def pinhole_raymat(H, W, f=None, origin=(0.1, -0.2, 0.3)):
    """rays_d(x, y) = ((x - cx) / f, (y - cy) / f, 1), rays_o = origin, as the kernels' float[12]."""
    f = float(max(H, W, 8)) if f is None else f
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([1 / f, 0, 0, 0, 1 / f, 0, -cx / f, -cy / f, 1, *origin], np.float32)


def surface_scene(H, W, seed, raymat=None):
    """allmap [8, H, W] float32 of a sphere in front of a tilted plane, alpha varied in [0.05, 1], depth sum = depth * alpha,
    median depth a slightly different surface; the unused planes hold noise (they get no gradient)."""
    rs = np.random.RandomState(seed)
    ray = pinhole_raymat(H, W) if raymat is None else np.asarray(raymat, np.float32)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xs * ray[0] + ys * ray[3] + ray[6], xs * ray[1] + ys * ray[4] + ray[7]
    depth = 4.0 + 0.8 * dx - 0.5 * dy
    r2 = dx * dx + dy * dy
    depth = np.where(r2 < 0.09, 3.0 - np.sqrt(np.maximum(0.09 - r2, 0)) * 2.0, depth)
    alpha = 0.05 + 0.95 * rs.rand(H, W)
    am = rs.rand(8, H, W)
    am[1] = alpha
    am[0] = depth * alpha * (1 + 1e-3 * rs.randn(H, W))
    am[5] = depth + 0.01 * rs.randn(H, W)
    return np.ascontiguousarray(am, np.float32), np.asarray(ray, np.float32)


def surface_branch_scene(H, W, seed, depth_ratio):
    """The surface pass's rare branches in one map: alpha 0, one ulp below / at / above the clamp; +inf, -inf and NaN in the
    depth and median planes (-inf only where the ratio gives it weight 0: elsewhere its float32 lowest overflows the points);
    a band of depths tiny enough that the cross product is shorter than 1e-12 (camera at the origin, so the points do not
    round away); a band of zero depth, where the cross product is exactly 0."""
    rs = np.random.RandomState(seed)
    ray = pinhole_raymat(H, W, origin=(0.0, 0.0, 0.0))
    am, _ = surface_scene(H, W, seed, ray)
    alpha, depth = am[1].astype(np.float64), (am[0] / am[1]).astype(np.float64)
    # alpha at the clamp: every fourth column cycles through the four cases
    cols = np.arange(W)
    for k, a in enumerate(ALPHA_CASES):
        sel = (cols % 8 == 2 * k + 1)[None, :] & (np.arange(H) % 3 == 1)[:, None]
        alpha = np.where(sel, a, alpha)
    # tiny depths (|c| ~ 1e-20) in the rows y % 9 == 4 .. 6; exact zero depth in the rows y % 9 == 7
    rows = np.arange(H)[:, None] % 9
    depth = np.where((rows >= 4) & (rows <= 6), 1e-5 * (1 + 0.1 * rs.rand(H, W)), depth)
    depth = np.where(rows == 7, 0.0, depth)
    am[1] = alpha
    am[0] = depth * alpha
    am[5] = np.where(rows == 7, 0.0, depth)
    # non-finite values at chosen pixels
    pix = [(y, x) for y in range(H) for x in range(W) if (y * 7 + x * 3) % 23 == 5]
    for i, (y, x) in enumerate(pix):
        kind = i % 4
        if kind == 0:
            am[0, y, x] = np.inf
        elif kind == 1:
            am[0, y, x] = np.nan
        elif kind == 2:
            am[5, y, x] = [np.inf, np.nan][(i // 4) % 2]
        else:
            if depth_ratio == 1.0:
                am[0, y, x] = -np.inf
            elif depth_ratio == 0.0:
                am[5, y, x] = -np.inf
            else:
                am[5, y, x] = np.nan
    return np.ascontiguousarray(am, np.float32), ray
