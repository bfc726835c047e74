"""References for the viewer presentation (csrc/gsr_viewer.hip, utils/image_utils.py); not a test.

Three statements of the same thing:

  * `torch_chain`: the reference's float32 chain on the CPU, written out from utils/image_utils.py:33-84 (render_net_image, colormap,
    gradient_map: F.conv2d per channel with padding 1) and train.py:334 (clamp, times 255, .byte(), to [H, W, 3]).  Two places where
    the reference itself fails are defined here as the product defines them: a map with max == min takes index 0 (the reference
    divides by zero), and the index plane is reshaped to [H, W] (the reference's squeeze() also drops a height or width of 1).
  * `restate`: numpy.  The pointwise modes in float32, operation by operation (IEEE arithmetic: bit for bit what torch computes); the
    colour index for either precision; `gradient_reference` in float64 with a running error bound.
  * the kernel, held to the first bit for bit wherever the order of the float32 operations is fixed, and to the float64 gradient within
    its bound where it is not (a 3x3 convolution may be summed in any order).

The bound of the gradient.  u = 2**-24; all errors absolute.  With p the image after the affine (x + 1) / 2 (one rounding, of x + 1;
the halving is exact) and zero outside the image:
    e_p   = u |p|                              (0 without the affine)
    g     = sum_k w_k p_k                      six non-zero weights, each +-1/4 or +-1/2: the products are exact
    e_g   = sum_k |w_k| e_p_k + 5 u sum_k |w_k| |p_k|        five additions, in any order: every partial sum is at most the sum of magnitudes
    m     = sqrt(gx^2 + gy^2), 1-Lipschitz in (gx, gy):   e_m = hypot(e_gx, e_gy) + 3 u m     (two squares, a sum, a root: at most 2.5 u m)
    out   = sqrt(sum_c m_c^2):                             e_out = sqrt(sum_c e_m_c^2) + 3 u out
    bound = K_GRAD e_out, K_GRAD = 2 for what first order drops, as tests/loss_bounds.py does.

The bound of the colour index.  s = 255 (x - min) / (max - min); with R = max - min, b the gradient's bound at the pixel and B its
largest value over the image (min and max may come from any pixel):
    |ds| <= 255 / R (b + B + (s / 255) 2 B) + 3 u 255        (the subtraction, the division, the product: one rounding each)
A pixel is near a boundary when s lies within that of k + 1/2: there, and only there, the float32 index may be one level off.
"""
import numpy as np

U = 2.0 ** -24
K_GRAD = 2.0
NEAR_CAP = 0.01            # at most this share of the pixels may take the one-level exception

SHAPES = ((1, 1), (1, 7), (7, 1), (5, 3), (33, 31), (64, 65), (75, 101))      # (H, W): a four-pixel lane, a 64-lane row, a halo tile
FULL_SIZE = (1080, 1920)
SOBEL_SHAPES = ((33, 31), (64, 65), (75, 101))
FAMILIES = ("smooth", "normals", "constant", "two_valued", "out_of_range", "nan")

# every mode string of render_net_image, in the order a viewer might list them; "RGB" is the fallback (rgb_out)
ITEMS = ["RGB", "Alpha", "Normal", "Depth", "Base Color", "Refl. Strength", "Refl. Color", "Edge", "Curvature", "Mask", "RGB raw"]
# lower-case mode -> (key of the render package, channels, affine, sobel, repeated)
MODES = {
    "alpha": ("rend_alpha", 1, False, False, False),
    "mask": ("env_scope_mask", 1, False, False, True),
    "normal": ("rend_normal", 3, True, False, False),
    "depth": ("surf_depth", 1, False, False, False),
    "base color": ("base_color_map", 3, False, False, False),
    "refl. strength": ("refl_strength_map", 1, False, False, True),
    "refl. color": ("refl_color_map", 3, False, False, False),
    "edge": ("surf_normal", 3, True, False, False),
    "curvature": ("rend_normal", 3, True, True, False),
    "rgb raw": ("render", 3, False, False, False),
}
PACKAGE = {"render": 3, "rend_alpha": 1, "rend_normal": 3, "surf_depth": 1, "base_color_map": 3, "refl_strength_map": 1,
           "refl_color_map": 3, "surf_normal": 3, "env_scope_mask": 1}


def turbo():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return np.loadtxt(os.path.join(root, "gaussian-splatting-reflection_amd", "utils", "turbo_lut.txt"), dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- inputs
def image(family, C, H, W, seed):
    """float32 [C, H, W] of an input family."""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    if family == "smooth":
        ph = rs.rand(C, 3) * 6.0
        v = np.stack([0.5 + 0.3 * np.sin(0.11 * xs + ph[c, 0]) * np.cos(0.07 * ys + ph[c, 1]) + 0.15 * np.sin(0.013 * (xs + ys) + ph[c, 2])
                      for c in range(C)])
    elif family == "normals":              # noisy unit normals (one channel: noise in [-1, 1])
        v = rs.randn(C, H, W) + np.array([0.0, 0.0, 1.5][:C]).reshape(C, 1, 1)
        v = v / np.sqrt((v * v).sum(0, keepdims=True)) if C == 3 else np.clip(0.5 * v, -1, 1)
    elif family == "constant":
        v = np.full((C, H, W), 0.37) * np.array([1.0, -0.5, 2.0][:C]).reshape(C, 1, 1)
    elif family == "two_valued":
        v = np.where(rs.rand(C, H, W) < 0.5, 0.25, 0.75)
    elif family == "out_of_range":
        v = -0.5 + 2.0 * rs.rand(C, H, W)
    elif family == "nan":
        v = 0.1 + 0.8 * rs.rand(C, H, W)
        v[C // 2, H // 2, W // 2] = np.nan
    else:
        raise ValueError(family)
    return np.ascontiguousarray(v, np.float32)


def package(family, H, W, seed):
    """(rgb_out, render package) of numpy arrays: every key a mode reads, each with its own seed."""
    pkg = {k: image(family, C, H, W, seed + 7 * i) for i, (k, C) in enumerate(sorted(PACKAGE.items()))}
    return image(family, 3, H, W, seed + 101), pkg


def select(rgb_out, pkg, items, mode):
    """(source, affine, sobel, repeated) by the reference's rules; KeyError where the package lacks the key."""
    if mode >= len(items):
        mode = 0
    m = MODES.get(items[mode].lower())
    if m is None:
        return rgb_out, False, False, False
    key, _, half, sobel, repeated = m
    return pkg[key], half, sobel, repeated


def colour_mapped(items, mode):
    m = MODES.get(items[mode if mode < len(items) else 0].lower())
    return m is not None and not m[4] and (m[1] == 1 or m[3])


def defined(family, items, mode, H, W):
    """Whether the reference's chain defines the mode on the family: a NaN under a colour map does not (its min and max are NaN)."""
    return not (family == "nan" and colour_mapped(items, mode))


# ------------------------------------------------------------------------------------------------------- numpy restatement
def colour_index(x, dtype):
    """colormap()'s index plane of x [H, W] in `dtype` arithmetic: round half to even of (x - min) / (max - min) * 255; all zeros
    where max == min."""
    x = np.asarray(x, dtype)
    mn, mx = x.min(), x.max()
    if not mx > mn:
        return np.zeros(x.shape, np.int64)
    with np.errstate(invalid="ignore"):
        s = ((x - mn) / (mx - mn)).astype(dtype) * dtype(255)
    return np.rint(s.astype(dtype)).astype(np.int64)


def frame_bytes(img):
    """train.py:334 on float32 [3 or 1, H, W]: trunc(clamp(img, 0, 1) * 255) as [H, W, 3]; a NaN gives 0."""
    v = np.asarray(img, np.float32)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1)))
    b = (v * np.float32(255)).astype(np.float32).astype(np.uint8)
    if b.shape[0] == 1:
        b = np.repeat(b, 3, 0)
    return np.ascontiguousarray(b.transpose(1, 2, 0))


_WX = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64) / 4
_WY = _WX.T.copy()


def _corr3(w, P, H, W):
    out = np.zeros((H, W))
    for i in range(3):
        for j in range(3):
            if w[i, j] != 0.0:
                out += w[i, j] * P[i:i + H, j:j + W]
    return out


def gradient_reference(x32, half=False):
    """gradient_map in float64 on float32 input [C, H, W] (after the affine when `half`), and the bound of the module docstring.
    Returns (magnitude [1, H, W], bound [1, H, W])."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    C, H, W = x.shape
    p = (x + 1.0) / 2.0 if half else x
    e_p = U * np.abs(p) if half else np.zeros_like(p)
    out2, e2 = np.zeros((H, W)), np.zeros((H, W))
    for c in range(C):
        P, A, E = (np.pad(t, 1) for t in (p[c], np.abs(p[c]), e_p[c]))
        gx, gy = _corr3(_WX, P, H, W), _corr3(_WY, P, H, W)
        e_gx = _corr3(np.abs(_WX), E, H, W) + 5 * U * _corr3(np.abs(_WX), A, H, W)
        e_gy = _corr3(np.abs(_WY), E, H, W) + 5 * U * _corr3(np.abs(_WY), A, H, W)
        m = np.hypot(gx, gy)
        e_m = np.hypot(e_gx, e_gy) + 3 * U * m
        out2 += m * m
        e2 += e_m * e_m
    out = np.sqrt(out2)
    return out[None], (K_GRAD * (np.sqrt(e2) + 3 * U * out))[None]


def index_reference(ref, bound):
    """The float64 colour index of a plane [H, W] known within `bound`, and the mask of pixels near a rounding boundary (see the
    module docstring).  max == min: zeros, and no pixel is near."""
    ref, bound = np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    mn, mx = ref.min(), ref.max()
    R = mx - mn
    if not R > 0:
        return np.zeros(ref.shape, np.int64), np.zeros(ref.shape, bool), np.zeros(ref.shape)
    s = (ref - mn) / R * 255.0
    B = bound.max()
    delta = 255.0 / R * (bound + B + (s / 255.0) * 2 * B) + 3 * U * 255.0
    near = np.abs(s - (np.floor(s) + 0.5)) <= delta
    return np.rint(s).astype(np.int64), near, delta


def restate(rgb_out, pkg, items, mode, table):
    """dict(img float32 [3, H, W], frame uint8 [H, W, 3], exact) of a mode; with Sobel also idx, near, grad, bound (float64), and
    exact is False: img and frame are the table at the float64 index."""
    src, half, sobel, repeated = select(rgb_out, pkg, items, mode)
    src = np.asarray(src, np.float32)
    if sobel:
        grad, bound = gradient_reference(src, half)
        idx, near, _ = index_reference(grad[0], bound[0])
        img = np.ascontiguousarray(table[idx].transpose(2, 0, 1))
        return dict(img=img, frame=frame_bytes(img), exact=False, idx=idx, near=near, grad=grad, bound=bound)
    x = ((src + np.float32(1)) / np.float32(2)).astype(np.float32) if half else src
    if repeated:
        img = np.repeat(x, 3, 0)
    elif x.shape[0] == 1:
        idx = colour_index(x[0], np.float32)
        img = np.ascontiguousarray(table[idx].transpose(2, 0, 1))
        return dict(img=img, frame=frame_bytes(img), exact=True, idx=idx)
    else:
        img = x
    return dict(img=img, frame=frame_bytes(img), exact=True)


# ------------------------------------------------------------------------------------------------- the float32 torch chain
def torch_gradient_map(image):
    """utils/image_utils.py:33-42 on a float32 CPU tensor [C, H, W]."""
    import torch
    import torch.nn.functional as F
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]).reshape(1, 1, 3, 3) / 4
    ky = kx.transpose(2, 3).contiguous()
    gx = torch.cat([F.conv2d(image[c][None], kx, padding=1) for c in range(image.shape[0])])
    gy = torch.cat([F.conv2d(image[c][None], ky, padding=1) for c in range(image.shape[0])])
    return torch.sqrt(gx ** 2 + gy ** 2).norm(dim=0, keepdim=True)


def torch_colormap(m, table):
    """utils/image_utils.py:44-49 on [1, H, W] with the table as a tensor; max == min: index 0."""
    import torch
    mn, mx = m.min(), m.max()
    if not bool(mx > mn):
        idx = torch.zeros(m.shape[1:], dtype=torch.long)
    else:
        idx = (((m - mn) / (mx - mn)) * 255).round().long().reshape(m.shape[1:])
    return table[idx].permute(2, 0, 1), idx


def torch_chain(rgb_out, pkg, items, mode, table):
    """(float image [3, H, W], frame uint8 [H, W, 3], index plane or None, gradient or None) as numpy, computed by torch in float32 on
    the CPU the way the reference's render_net_image and train.py:334 do."""
    import torch
    src, half, sobel, repeated = select(rgb_out, pkg, items, mode)
    img = torch.from_numpy(np.ascontiguousarray(src, np.float32))
    idx = grad = None
    if half:
        img = (img + 1) / 2
    if sobel:
        img = grad = torch_gradient_map(img)
    if repeated:
        img = img.repeat(3, 1, 1)
    if img.shape[0] == 1:
        img, idx = torch_colormap(img, torch.from_numpy(table))
    frame = (torch.clamp(img, min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous()
    return (img.contiguous().numpy(), frame.numpy(), None if idx is None else idx.numpy(), None if grad is None else grad.numpy())


def check_indices(got, ref_idx, near, what=""):
    """Every index equals the float64 index, or is one level off at a pixel near a rounding boundary; at most NEAR_CAP of the pixels
    take the exception.  Returns the share that did."""
    got, ref_idx = np.asarray(got, np.int64), np.asarray(ref_idx, np.int64)
    off = got != ref_idx
    bad = off & ~((np.abs(got - ref_idx) == 1) & near)
    assert not bad.any(), f"{what}: {int(bad.sum())} indices differ away from a rounding boundary, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"got {got[tuple(np.argwhere(bad)[0])]}, float64 {ref_idx[tuple(np.argwhere(bad)[0])]}"
    share = float(off.mean())
    assert share <= NEAR_CAP, f"{what}: {share:.4f} of the pixels took the one-level exception, cap {NEAR_CAP}"
    return share


# ---------------------------------------------------------------------------------------- numpy restatements of the layouts
def cubemap_cross(textures):
    """plot_cubemap: six faces [6, C, h, w] in the 4 x 3 cross; cell k at row k // 4, column k % 4."""
    t = np.asarray(textures)
    _, C, h, w = t.shape
    out = np.zeros((C, 3 * h, 4 * w), t.dtype)
    for cell, face in {1: t[3][:, ::-1, :], 4: t[1], 5: t[4], 6: t[0], 7: t[5], 9: t[2]}.items():
        r, c = divmod(cell, 4)
        out[:, r * h:(r + 1) * h, c * w:(c + 1) * w] = face
    return np.repeat(out, 3, 0) if C == 1 else out


def three_channels(a):
    """to_3ch on a numpy array: [B, 3, H, W]."""
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[None, None]
    elif a.ndim == 3:
        a = a[None] if a.shape[0] in (1, 3) else a.transpose(2, 0, 1)[None]
    elif a.shape[1] not in (1, 3) and a.shape[3] in (1, 3):
        a = a.transpose(0, 3, 1, 2)
    if a.shape[1] != 3:
        a = np.repeat(a.mean(1, keepdims=True) if a.shape[1] != 1 else a, 3, 1)
    return a
