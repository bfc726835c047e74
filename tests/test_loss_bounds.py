"""The error bounds of tests/loss_bounds.py, checked on the CPU with the float32 oracle as a second float32 implementation:
not too tight (the float32 oracle stays inside at every element), not vacuous (a high quantile of bound / |reference| is
small on natural content) and able to catch an error (one element just outside its bound is rejected)."""
import numpy as np
import pytest

import loss_bounds as LB
from oracle import oracle as orc

W_L1, W_SSIM = 0.8, -0.2


def _ssim_f32(x, y):
    l1, ss, m = orc.ssim_l1_forward(x, y, LB.C1, LB.C2, dtype=np.float32)
    g = orc.ssim_l1_backward(x, y, np.float32(W_L1), np.float32(W_SSIM), LB.C1, LB.C2, dtype=np.float32)
    return dict(l1=l1, ssim=ss, map=m, grad=g)


@pytest.mark.parametrize("family", LB.FAMILIES)
def test_ssim_bounds_hold_for_the_float32_oracle(family):
    for shape in [(3, 37, 65), (2, 64, 33), (1, 6, 11)]:
        x, y = LB.loss_pair(family, shape, 1)
        ref, bnd = LB.ssim_reference(x, y, W_L1, W_SSIM)
        got = _ssim_f32(x, y)
        for k in ("l1", "ssim", "map", "grad"):
            LB.check(got[k], ref[k], bnd[k], what=f"{family} {shape} {k}")


def test_ssim_bounds_are_not_vacuous():
    """On noise images the map is held to ~1e-4 of its value: the variances (~0.05) are differences of second moments
    (~0.3), so even the exact float32 evaluation keeps only ~3 fewer bits than the inputs.  The gradient is a signed sum that
    passes through zero, so its median (not a high quantile) of bound / |reference| is held."""
    for family in ("uniform", "checker"):
        x, y = LB.loss_pair(family, (3, 64, 96), 2)
        ref, bnd = LB.ssim_reference(x, y, W_L1, W_SSIM)
        assert np.percentile(bnd["map"] / np.abs(ref["map"]), 99) < 2.5e-4, family
        assert np.median(bnd["grad"] / np.abs(ref["grad"])) < 1e-3, family
        assert bnd["l1"] < 1e-5 * ref["l1"] and bnd["ssim"] < 1e-4 * abs(ref["ssim"]), family


def test_ssim_bounds_reject_an_error_just_outside():
    x, y = LB.loss_pair("uniform", (2, 40, 50), 3)
    ref, bnd = LB.ssim_reference(x, y, W_L1, W_SSIM)
    for k in ("map", "grad"):
        bad = ref[k].copy()
        bad[1, 17, 33] += 1.01 * bnd[k][1, 17, 33]
        with pytest.raises(AssertionError):
            LB.check(bad, ref[k], bnd[k], what=k)
        ok = ref[k].copy()
        ok[1, 17, 33] += 0.99 * bnd[k][1, 17, 33]
        LB.check(ok, ref[k], bnd[k], what=k)
    with pytest.raises(AssertionError):
        LB.check(ref["ssim"] + 1.01 * bnd["ssim"], ref["ssim"], bnd["ssim"])


def _surface_cases():
    for (H, W) in [(34, 33), (18, 31), (3, 4), (17, 16)]:
        for ratio in (0.0, 0.3, 1.0):
            for mode in ("both", "depth_only", "normal_only"):
                yield H, W, ratio, mode


def _cot(H, W, mode, seed):
    rs = np.random.RandomState(seed)
    gsd = rs.randn(H, W).astype(np.float32) if mode != "normal_only" else None
    gsn = rs.randn(3, H, W).astype(np.float32) if mode != "depth_only" else None
    return gsd, gsn


@pytest.mark.parametrize("scene", ["smooth", "branches"])
def test_surface_bounds_hold_for_the_float32_oracle(scene):
    for k, (H, W, ratio, mode) in enumerate(_surface_cases()):
        am, ray = LB.surface_scene(H, W, k) if scene == "smooth" else LB.surface_branch_scene(H, W, k, ratio)
        gsd, gsn = _cot(H, W, mode, k)
        ref, bnd, skip = LB.surface_reference(am, ray, ratio, gsd, gsn)
        sd, sn, g = orc.surface_pass(am, ray, np.float32(ratio), gsd, gsn, dtype=np.float32)
        what = f"{scene} {H}x{W} ratio={ratio} {mode}"
        LB.check(sd, ref["sd"], bnd["sd"], skip["sd"], what + " sd")
        LB.check(sn, ref["sn"], bnd["sn"], skip["sn"], what + " sn")
        LB.check(g, ref["g"], bnd["g"], skip["g"], what + " g")
        assert not skip["g"].any() or scene == "branches"


def test_surface_bounds_are_not_vacuous_and_reject_errors():
    am, ray = LB.surface_scene(40, 48, 7)
    gsd, gsn = _cot(40, 48, "both", 7)
    ref, bnd, skip = LB.surface_reference(am, ray, 0.3, gsd, gsn)
    inner = (slice(None), slice(1, -1), slice(1, -1))
    assert np.percentile(bnd["sd"] / np.abs(ref["sd"]), 99) < 1e-6
    assert np.percentile(bnd["sn"][inner] / np.abs(ref["sn"][inner]), 99) < 5e-3     # normals of points ~1/48 apart: cancellation
    for p in (0, 1, 5):                        # the same cross products, differentiated: a few times the normals' median
        assert np.median(bnd["g"][p] / np.abs(ref["g"][p])) < 3e-3
    for key, idx in (("sd", (20, 21)), ("sn", (2, 20, 21)), ("g", (1, 20, 21)), ("g", (0, 1, 47)), ("g", (5, 39, 0))):
        bad = ref[key].copy()
        bad[idx] += 1.01 * bnd[key][idx]
        with pytest.raises(AssertionError):
            LB.check(bad, ref[key], bnd[key], skip[key], key)


def test_surface_non_finite_classes_and_fp32_constants():
    """The float64 oracle uses the float32 constants: nan_to_num(-inf) is the float32 lowest, the clamp is fl32(1e-3).  NaN
    and infinity classes are compared as classes."""
    H, W = 5, 6
    am = np.zeros((8, H, W), np.float32)
    am[1] = 0.5
    am[0] = 1.0
    am[5] = 2.0
    am[0, 2, 2] = -np.inf
    am[5, 2, 3] = -np.inf
    am[1, 1, 1] = np.float32(LB.ALPHA_MIN) * np.float32(0.5)
    ray = LB.pinhole_raymat(H, W)
    for dt in (np.float32, np.float64):
        sd, _, g = orc.surface_pass(am, ray, 0.0, np.ones((H, W), np.float32), None, dtype=dt, fp32_constants=True)
        assert sd[2, 2] == -np.finfo(np.float32).max and np.isnan(g[1, 2, 2])
        assert sd[1, 1] == (np.float32(1.0) / np.float32(LB.ALPHA_MIN) if dt == np.float32 else 1.0 / LB.ALPHA_MIN)
    # without fp32_constants the float64 path is the chain run on float64 tensors (tests/golden/surface_golden.npz)
    sd64, _, _ = orc.surface_pass(am, ray, 0.0, dtype=np.float64)
    assert sd64[2, 2] == np.finfo(np.float64).min and sd64[1, 1] == 1.0 / 1e-3
    ref = np.array([np.nan, np.inf, -np.inf, 1.0])
    LB.check(np.array([np.nan, np.inf, -np.inf, 1.0]), ref, np.zeros(4))
    for wrong in ([0.0, np.inf, -np.inf, 1.0], [np.nan, -np.inf, -np.inf, 1.0], [np.nan, np.inf, np.nan, 1.0]):
        with pytest.raises(AssertionError):
            LB.check(np.array(wrong), ref, np.zeros(4))


def test_adam_bounds():
    rs = np.random.RandomState(4)
    n = 5000
    p = rs.randn(n).astype(np.float32)
    g = (rs.randn(n) * 10.0 ** rs.uniform(-6, 1, n)).astype(np.float32)
    m = (rs.randn(n) * 0.1).astype(np.float32)
    v = (rs.rand(n) * 0.01).astype(np.float32)
    lr = np.where(np.arange(n) % 7 < 3, 0.0025, 0.0025 / 20).astype(np.float32)
    for step in (1, 2, 30_000):
        ref, bnd = LB.adam_reference(p, g, m, v, lr, 0.9, 0.999, 1e-15, step)
        got = orc.adam(p, g, m, v, lr, beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)), eps=float(np.float32(1e-15)), step=step,
                       dtype=np.float32)
        for k in range(3):
            LB.check(got[k], ref[k], bnd[k], what=f"step {step} {k}")
        assert np.percentile(bnd[0] / np.abs(ref[0]), 99) < 1e-6
        bad = ref[0].copy()
        bad[123] += 1.01 * bnd[0][123]
        with pytest.raises(AssertionError):
            LB.check(bad, ref[0], bnd[0])
