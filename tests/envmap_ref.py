"""Float64 numpy restatement of the two environment-map entries (include/gsr_hip_envmap.h), written from their contracts: what
tests/test_cabi_envmap.py's library is compared with in tests/test_gpu_envmap.py, and what tests/test_envmap_ref.py pins against torch's
own bicubic interpolation and this project's _adjust_sharpness.  No torch here: arrays in, float64 arrays out."""
import numpy as np

A = -0.75
LO, HI = 1e-3, 1 - 1e-3          # the reference's clamp (cubemap_encoder.py:112)
# the two derived bounds of tests/test_gpu_envmap.py (worst cases, not measurements)
RESIZE_REL_BOUND = 4e-5          # |out - ref| <= 4e-5 * max|src|: degree-3 Horner weights with intermediates up to 6, one rounding in the fraction, 16 taps
SHARPEN_ACT_BOUND = 4e-6         # in activated space: float32 exp, a 10-term sum of values in [0, 1], a blend of magnitude at most 3


def cubic_weights(t):
    """The four weights of the taps at i-1 .. i+2 for the fraction t (scalar or array; the result has a last axis of 4)."""
    t = np.asarray(t, dtype=np.float64)

    def near(x):
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def far(x):
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.stack([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)], axis=-1)


def source_coords(L_src, L_dst):
    """(i [L_dst] int64, t [L_dst] float64): the source node and the fraction of every output node, from integers."""
    d = np.arange(L_dst, dtype=np.int64)
    if L_dst == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.float64)
    n = d * (L_src - 1)
    return n // (L_dst - 1), (n % (L_dst - 1)).astype(np.float64) / float(L_dst - 1)


def resize(src, L_dst):
    """src [..., L_src, L_src] -> [..., L_dst, L_dst]: bicubic, align_corners=True, taps clamped, x first and then y."""
    src = np.asarray(src, dtype=np.float64)
    L_src = src.shape[-1]
    assert src.shape[-2] == L_src
    i, t = source_coords(L_src, L_dst)
    w = cubic_weights(t)                                                       # [L_dst, 4]
    taps = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, L_src - 1)       # [L_dst, 4]
    along_x = sum(src[..., :, taps[:, k]] * w[:, k] for k in range(4))         # [..., L_src, L_dst]
    return sum(along_x[..., taps[:, k], :] * w[:, k][:, None] for k in range(4))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def sharpen_activated(src, factor, lo=LO, hi=HI):
    """The clamped activated value `o` of every texel of src [..., L, L]."""
    s = sigmoid(src)
    L = s.shape[-1]
    o = s.copy()
    if L > 2:
        total = np.zeros_like(s[..., 1:-1, 1:-1])
        for dy in range(3):
            for dx in range(3):
                total = total + s[..., dy:dy + L - 2, dx:dx + L - 2]
        centre = s[..., 1:-1, 1:-1]
        b = (total + 4.0 * centre) / 13.0
        o[..., 1:-1, 1:-1] = np.clip(factor * centre + (1.0 - factor) * b, 0.0, 1.0)
    return np.clip(o, lo, hi)


def sharpen(src, factor, lo=LO, hi=HI):
    o = sharpen_activated(src, factor, lo, hi)
    return np.log(o / (1.0 - o))
