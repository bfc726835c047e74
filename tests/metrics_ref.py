"""Float64 references with error bounds for the evaluation metrics (csrc/gsr_metrics.hip, gsr_eval.py), in the manner of
tests/loss_bounds.py, plus the seeded inputs their tests use.

Presentation (render.py:48-62 and the PNG round trip of save_image / to_tensor) is restated in float64 from the same float32 inputs
with every operation rounded to float32 as the torch chain rounds it: a product of two float32 values is exact in float64, so is a
sum of two whose exponents lie within 29 binades, and one cast rounds it correctly.  The presented images are therefore the exact
float32 values the kernel must stage, and the 8-bit images must be equal, not close.

The three sums and the angular error are bounded as

    |result - float64 reference| <= K * u * kappa,        u = 2**-24

with kappa the running-error estimate of the expression (tests/loss_bounds.py explains the rules).  The SSIM sum takes its reference,
its kappa and its K from loss_bounds.  The other constants are twice the worst observed error / (u * kappa) of the kernels over the
cases of tests/test_gpu_metrics.py on an MI355X, the factor covering compiler and clock-state variation.  The measured value stands
beside each K.  No element is excused anywhere.
"""
import os

import numpy as np

import loss_bounds as LB

U = LB.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mae_reference.npz")

NSUM = LB.NSUM          # additions a pixel's term passes through in the image kernel's block reduction (as the loss kernel's)
# K = 2 x the worst |error| / (u * kappa) measured on an MI355X over every comparison of tests/test_gpu_metrics.py (the sums' errors
# behave like random walks inside a worst-case kappa, hence constants below 1)
K_SSE = 0.16            # sum (v - g)^2   measured worst 0.076 (quantizer_edges, mask_only, 3x5x7)
K_SAD = 0.16            # sum |v - g|     measured worst 0.078 (uniform, none, 3x33x31)
K_SSIM = LB.K_SUM       # sum ssim_map    loss_bounds' constant, 2; measured worst 0.038 (constants, mask_only, 3x43x75)
K_ANGLE = 1.8           # angle per pixel measured worst 0.89 (degenerate, 1080x1920)
K_ANGLE_SUM = 0.7       # sum of angles   measured worst 0.35 (identical, 1x1)
NACOS = 4               # roundings granted to acosf itself (its documented error is below 2 ulp) and the conversion to degrees
DEG = 180.0 / np.pi


def f32(a):
    """One float32 rounding of a float64 array, returned as float64."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- presentation
def clamp01(t):
    return np.clip(t, 0.0, 1.0)


def composite(t, a, bg):
    """t * a + (1 - a) * bg[c] with the four float32 roundings of the torch expression; t [C,H,W], a [H,W], bg [C] (float64 holding
    float32 values)."""
    b = np.asarray(bg, np.float64).reshape(-1, 1, 1)
    return f32(f32(t * a[None]) + f32(f32(1.0 - a[None]) * b))


# (t, alpha, channel) with background COMPOSITE_BG at which t * a + (1 - a) * bg rounded as torch rounds it (four operations) and with
# either product folded into a fused multiply-add land on opposite sides of a quantiser threshold: the 8-bit level tells the two apart.
# Found by a seeded search over uniform float32 inputs; tests/test_metrics_ref.py checks every one of them against torch.
COMPOSITE_BG = (0.1, 0.95, 0.3)
COMPOSITE_EDGES = (          # the first four differ under fma(t, a, (1 - a) * bg), the last four under fma(1 - a, bg, t * a)
    ("0x1.62ef88p-1", "0x1.85081ap-1", 1), ("0x1.786630p-1", "0x1.fb8cccp-1", 2), ("0x1.fda7f4p-2", "0x1.2cc31ap-1", 1),
    ("0x1.06fbe4p-1", "0x1.8153d4p-1", 2), ("0x1.892478p-3", "0x1.bbaa28p-2", 1), ("0x1.3cc088p-1", "0x1.f9fc2ep-2", 1),
    ("0x1.62ef88p-1", "0x1.85081ap-1", 1), ("0x1.431dd0p-2", "0x1.b7e37ep-3", 1))


def composite_edge_image():
    """(img [3,4,4], alpha [4,4], background [3]) float32 holding COMPOSITE_EDGES, one per pixel, in its channel; 0.5 elsewhere."""
    img = np.full((3, 4, 4), 0.5, np.float32)
    alpha = np.full(16, 0.25, np.float32)
    for i, (t, a, c) in enumerate(COMPOSITE_EDGES):
        img[c, i // 4, i % 4] = np.float32(float.fromhex(t))
        alpha[i] = np.float32(float.fromhex(a))
    return img, alpha.reshape(4, 4), np.array(COMPOSITE_BG, np.float32)


def composite_contracted(t, a, bg, which):
    """The composite with one product folded into an FMA (which = 0: t * a, 1: (1 - a) * bg): one rounding less."""
    b = np.asarray(bg, np.float64).reshape(-1, 1, 1)
    if which == 0:
        return f32(t * a[None] + f32(f32(1.0 - a[None]) * b))
    return f32(f32(1.0 - a[None]) * b + f32(t * a[None]))


def quantize_levels(t):
    """uint8(clamp(t * 255 + 0.5, 0, 255)) of float32 values as torch's float32 chain computes it (the integer levels)."""
    s = f32(f32(np.asarray(t, np.float64) * 255.0) + 0.5)
    return np.floor(np.clip(s, 0.0, 255.0)).astype(np.uint8)


def quantize8(t):
    """The level divided by 255 in float32: what to_tensor gives back."""
    return f32(quantize_levels(t).astype(np.float64) / 255.0)


def present(img, gt, clamp=False, alpha=None, gt_mask=None, background=None, quantize=False):
    """Both images as the kernel must stage them (float64 arrays of float32 values) and, with quantize, their 8-bit levels."""
    v, g = np.asarray(img, np.float32).astype(np.float64), np.asarray(gt, np.float32).astype(np.float64)
    if clamp:
        v = clamp01(v)
    if alpha is not None:
        v = composite(v, clamp01(np.asarray(alpha, np.float32).astype(np.float64).reshape(v.shape[1:])), background)
    if gt_mask is not None:
        g = composite(g, np.asarray(gt_mask, np.float32).astype(np.float64).reshape(g.shape[1:]), background)
    lv = lg = None
    if quantize:
        lv, lg = quantize_levels(v), quantize_levels(g)
        v, g = quantize8(v), quantize8(g)
    return v, g, lv, lg


def torch_present(img, gt, clamp=False, alpha=None, gt_mask=None, background=None, quantize=False):
    """The same with torch float32 operations on the CPU, written as render.py and save_image write them."""
    import torch
    v, g = torch.from_numpy(np.asarray(img, np.float32)), torch.from_numpy(np.asarray(gt, np.float32))
    bg = None if background is None else torch.from_numpy(np.asarray(background, np.float32))
    if clamp:
        v = torch.clamp(v, 0.0, 1.0)
    if alpha is not None:
        a = torch.clamp(torch.from_numpy(np.asarray(alpha, np.float32)).reshape(1, *v.shape[1:]), 0.0, 1.0)
        v = v * a + (1 - a) * bg[:, None, None]
    if gt_mask is not None:
        m = torch.from_numpy(np.asarray(gt_mask, np.float32)).reshape(1, *g.shape[1:])
        g = g * m + (1 - m) * bg[:, None, None]
    lv = lg = None
    if quantize:
        lv, lg = (t.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8) for t in (v, g))
        v, g = lv.to(torch.float32).div(255), lg.to(torch.float32).div(255)
        lv, lg = lv.numpy(), lg.numpy()
    return v.numpy(), g.numpy(), lv, lg


# ------------------------------------------------------------------------------------------------------------------ image sums
def image_sums_reference(v, g):
    """Float64 references and bounds of {sse, sad, ssim} on presented images v, g (float64 arrays of float32 values, [C,H,W])."""
    from oracle import oracle as orc
    v32, g32 = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(g, np.float32)
    d = v32.astype(np.float64) - g32.astype(np.float64)
    sse, sad = float((d * d).sum()), float(np.abs(d).sum())
    _, s_ss, _ = orc.ssim_l1_forward(v32, g32, LB.C1, LB.C2, dtype=np.float64)
    k_ss = 0.0
    for c in range(v32.shape[0]):
        d_sv, asv, _, _ = LB._ssim_channel(v32[c].astype(np.float64), g32[c].astype(np.float64), 1.0, 1.0)
        k_ss += d_sv.sum() + NSUM * asv.sum()
    # d = v - g rounds once (|d|), d * d once more (or not at all inside an FMA): 3 d^2 per pixel, then NSUM additions
    ref = dict(sse=sse, sad=sad, ssim=float(s_ss))
    bnd = dict(sse=K_SSE * U * ((NSUM + 3) * sse + sse), sad=K_SAD * U * ((NSUM + 1) * sad + sad), ssim=K_SSIM * U * (k_ss + abs(s_ss)))
    return ref, bnd


def psnr(sse, n):
    with np.errstate(divide="ignore"):
        return float(20.0 * np.log10(1.0 / np.sqrt(np.float64(sse) / n)))


def psnr_bound(sse, b_sse):
    """d psnr = (10 / ln 10) * d sse / sse."""
    return float("inf") if sse == 0 else 10.0 / np.log(10.0) * b_sse / sse


# --------------------------------------------------------------------------------------------------------------- angular error
def angular_error_reference(pred, gt, eps=1e-8, pred_divisor=1.0, gt_divisor=1.0):
    """utils/mae_utils.py:10-27 in float64 on float32 inputs [3,H,W] with the float32 eps and divisors the kernel receives.
    Returns (angle [H,W] with NaN at invalid pixels, bound [H,W], ambiguous [H,W]): ambiguous marks pixels whose norm lies within its
    own rounding error of eps, where either verdict is right (the tests place none there)."""
    e = float(np.float32(eps))
    p = np.asarray(pred, np.float32).astype(np.float64) / float(np.float32(pred_divisor))
    g = np.asarray(gt, np.float32).astype(np.float64) / float(np.float32(gt_divisor))
    with np.errstate(all="ignore"):
        ap, ag = np.abs(p), np.abs(g)
        d_p = ap if pred_divisor != 1.0 else np.zeros_like(p)          # the division rounds once
        d_g = ag if gt_divisor != 1.0 else np.zeros_like(g)
        prod = p * g
        dot = prod.sum(0)
        d_dot = (ap * d_g + ag * d_p + np.abs(prod)).sum(0) + 2 * np.abs(prod).sum(0)
        sp, sg = (p * p).sum(0), (g * g).sum(0)
        d_sp, d_sg = (2 * ap * d_p + p * p).sum(0) + 2 * sp, (2 * ag * d_g + g * g).sum(0) + 2 * sg
        n_p, n_g = np.sqrt(sp), np.sqrt(sg)
        d_np = np.where(n_p > 0, d_sp / (2 * np.where(n_p > 0, n_p, 1.0)), 0.0) + n_p
        d_ng = np.where(n_g > 0, d_sg / (2 * np.where(n_g > 0, n_g, 1.0)), 0.0) + n_g
        nn = n_p * n_g
        den = nn + e
        d_den = n_p * d_ng + n_g * d_np + nn + den
        c = dot / den
        d_c = d_dot / den + np.abs(dot) * d_den / (den * den) + np.abs(c)
        cc = np.clip(c, -1.0, 1.0)
        ang = np.arccos(cc) * DEG
        # acos's conditioning 1 / sqrt(1 - c^2), floored where the cosine's own error reaches the end of the interval: there the angle
        # moves by at most acos(1 - 2 E) ~ 2 sqrt(E) for an error E of the cosine
        cond = 1.0 / np.sqrt(np.maximum(1.0 - cc * cc, 4.0 * U * d_c))
        d_ang = (d_c * cond + NACOS * np.arccos(cc)) * DEG + ang
        invalid = (n_p <= e) | (n_g <= e) | np.isnan(ang)
        ambiguous = (np.abs(n_p - e) <= 4 * U * d_np) | (np.abs(n_g - e) <= 4 * U * d_ng)
    return np.where(invalid, np.nan, ang), np.where(invalid, 0.0, K_ANGLE * U * d_ang), ambiguous & np.isfinite(n_p) & np.isfinite(n_g)


def mae_blocks(HW):
    return min(1024, (HW + 255) // 256)


def angle_sum_reference(ang, bound):
    """Reference and bound of the kernel's row {sum over valid pixels, valid, invalid}; the counts are exact."""
    valid = ~np.isnan(ang)
    s = float(ang[valid].sum())
    HW = ang.size
    nsum = -(-HW // (mae_blocks(HW) * 256)) + 9        # a thread's own additions + 6 wave + 3 block levels
    b = float((bound[valid] / K_ANGLE).sum()) * K_ANGLE_SUM + K_ANGLE_SUM * U * (nsum * s + s)
    return s, int(valid.sum()), int((~valid).sum()), b


def check_scalar(got, ref, bound, what):
    """One number inside its bound; returns |error| / bound (0 when both are 0) for the measurement log."""
    err = abs(float(got) - float(ref))
    q = err / bound if bound > 0 else 0.0
    print(f"ratio {what}: {q:.3f}")
    assert err <= bound, f"{what}: got {got!r}, reference {ref!r}, |error| {err:.3e} > bound {bound:.3e}"
    return q


# -------------------------------------------------------------------------------------------------------------- seeded inputs
IMAGE_SHAPES = ((3, 1, 1), (3, 5, 7), (3, 32, 32), (3, 33, 31), (3, 43, 75), (1, 64, 96))
FULL_SIZE = (3, 1080, 1920)
IMAGE_FAMILIES = ("uniform", "identical", "constants", "out_of_range", "quantizer_edges")
VARIANTS = ("none", "clamp", "clamp_composite_quantize", "mask_only")


def quantizer_edge_values():
    """All 256 levels k / 255, the 255 thresholds (k + 0.5) / 255, and +-1, +-2 ulp around each, as float32."""
    base = np.concatenate([np.arange(256, dtype=np.float64) / 255.0, (np.arange(255, dtype=np.float64) + 0.5) / 255.0]).astype(np.float32)
    out = [base]
    for direction in (np.float32(-np.inf), np.float32(np.inf)):
        t = base
        for _ in range(2):
            t = np.nextafter(t, direction)
            out.append(t)
    return np.concatenate(out)          # 5 * 511 values


def image_pair(family, shape, seed):
    rs = np.random.RandomState(seed)
    C, H, W = shape
    if family == "uniform":
        g = rs.rand(C, H, W)
        v = 0.6 * g + 0.4 * rs.rand(C, H, W)
    elif family == "identical":
        g = rs.rand(C, H, W)
        v = g.copy()
    elif family == "constants":
        v, g = np.full(shape, 0.3), np.full(shape, 0.7)
    elif family == "out_of_range":          # a render is not clamped: negative values and values above 1
        g = rs.rand(C, H, W)
        v = -0.5 + 2.0 * rs.rand(C, H, W)
    elif family == "quantizer_edges":       # the edge set tiled over both images at different phases
        e = quantizer_edge_values()
        n = C * H * W
        v = np.resize(e, n).reshape(shape)
        g = np.resize(np.roll(e, 977), n).reshape(shape)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(g, np.float32)


def presentation_inputs(variant, shape, seed):
    """kwargs of present() / torch_present() / MetricsTable.image for a variant: alpha beyond [0, 1] in places, a soft mask."""
    rs = np.random.RandomState(seed + 7)
    C, H, W = shape
    bg = np.array([0.1, 0.95, 0.3], np.float32)[:C]
    if variant == "none":
        return dict()
    if variant == "clamp":
        return dict(clamp=True)
    if variant == "clamp_composite_quantize":
        alpha = (-0.1 + 1.2 * rs.rand(H, W)).astype(np.float32)
        mask = np.where(rs.rand(H, W) < 0.5, np.float32(1.0), rs.rand(H, W).astype(np.float32)).astype(np.float32)
        return dict(clamp=True, alpha=alpha, gt_mask=mask, background=bg, quantize=True)
    if variant == "mask_only":
        return dict(gt_mask=(rs.rand(H, W) < 0.7).astype(np.float32), background=bg)
    raise ValueError(variant)


MAE_SHAPES = ((1, 1), (7, 5), (65, 64))
MAE_FAMILIES = ("random", "identical", "opposite", "degenerate", "eps_straddle")


def _unit(rs, H, W):
    n = rs.randn(3, H, W)
    return n / np.linalg.norm(n, axis=0, keepdims=True)


def normal_pair(family, H, W, seed):
    """(pred, gt) float32 [3,H,W].  degenerate: zero vectors and NaN components at seeded pixels of either input; eps_straddle: norms
    of 1e-8 * (1 -+ 1e-3) and 1e-8 * {0.5, 2}, far outside the rounding of the float32 norm, on unit ground truth."""
    rs = np.random.RandomState(seed)
    g = _unit(rs, H, W)
    if family == "random":
        p = _unit(rs, H, W)
    elif family == "identical":
        p = g.copy()
    elif family == "opposite":
        p = -g
    elif family == "degenerate":
        p = _unit(rs, H, W)
        kind = rs.randint(0, 6, (H, W))
        p[:, kind == 1] = 0.0
        g[:, kind == 2] = 0.0
        p[0, kind == 3] = np.nan
        g[2, kind == 4] = np.nan
        if H * W == 1:
            p[:] = 0.0
    elif family == "eps_straddle":
        p = _unit(rs, H, W)
        scale = np.choose(rs.randint(0, 5, (H, W)), [1.0, 1e-8 * (1 - 1e-3), 1e-8 * (1 + 1e-3), 0.5e-8, 2e-8])
        p = p * scale[None]
    else:
        raise ValueError(family)
    return np.ascontiguousarray(p, np.float32), np.ascontiguousarray(g, np.float32)


def golden_cases():
    """The inputs recorded in tests/golden/mae_reference.npz (tests/make_mae_golden.py): name -> (pred, gt) for angular_error_map,
    and name -> (pred [1,3,H,W] in 0..255, gt [1,3,H,W] in 0..65535) for compute_mae."""
    maps = {f: normal_pair(f, 9, 11, 40 + i) for i, f in enumerate(MAE_FAMILIES)}
    rs = np.random.RandomState(77)
    scaled = {}
    for name, H, W in (("scaled_a", 9, 11), ("scaled_b", 16, 5)):
        p, g = _unit(rs, H, W), _unit(rs, H, W)
        scaled[name] = (np.round((p * 0.5 + 0.5) * 255.0).astype(np.float32)[None], np.round((g * 0.5 + 0.5) * 65535.0).astype(np.float32)[None])
    p, g = _unit(rs, 6, 6), _unit(rs, 6, 6)
    scaled["unit_range"] = (np.abs(p).astype(np.float32)[None], np.abs(g).astype(np.float32)[None])      # max <= 1: no rescale
    return maps, scaled
