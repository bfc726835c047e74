"""The evaluation metrics on a machine without a GPU: the float64 restatements of tests/metrics_ref.py against what the reference
computes, the quantiser restatement against torch's float32 chain bit for bit, psnr / mse against known answers, the C entries'
export and binding, and every refusal of the C ABI before any device work.

The angular error is checked against vectors recorded from the reference's utils/mae_utils.py (tests/golden/mae_reference.npz, written
by tests/make_mae_golden.py).  psnr and mse have no such vectors: the reference's utils/image_utils.py imports torchvision and
matplotlib at module level and cannot be imported here, so they are checked against answers derived by hand from its two-line formula.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
FAKE = 0x7f0000000000          # 256-byte aligned, never dereferenced: every call below must fail validation first


# ------------------------------------------------------------------------------------------------------- angular error
def _golden():
    return np.load(MR.GOLDEN)


@pytest.mark.parametrize("family", MR.MAE_FAMILIES)
def test_angular_error_restatement_matches_the_recorded_reference(family):
    """The reference's float32 torch result lies inside the float64 restatement's bound at every valid pixel, and marks the same
    pixels invalid."""
    z = _golden()
    p, g, out = z[f"map_{family}_pred"], z[f"map_{family}_gt"], z[f"map_{family}_out"]
    ang, bound, ambiguous = MR.angular_error_reference(p, g)
    assert not ambiguous.any()
    assert (np.isnan(out) == np.isnan(ang)).all()
    if family in ("degenerate", "eps_straddle"):
        assert np.isnan(ang).any() and (~np.isnan(ang)).any()
    LBcheck(out, ang, bound, family)
    if family == "identical":
        assert np.nanmax(ang) <= 0.1          # float32 normals: the cosine is 1 within rounding, the angle within sqrt of that
    if family == "opposite":
        assert np.nanmin(ang) >= 179.9


def LBcheck(got, ref, bound, what):
    import loss_bounds as LB
    return LB.check(got, ref, bound, what=what)


def test_golden_inputs_are_the_seeded_cases():
    """The fixture holds the inputs metrics_ref.golden_cases() generates: re-recording reproduces it, and the GPU tests use the same."""
    z = _golden()
    maps, scaled = MR.golden_cases()
    for name, (p, g) in maps.items():
        np.testing.assert_array_equal(z[f"map_{name}_pred"], p)
        np.testing.assert_array_equal(z[f"map_{name}_gt"], g)
    for name, (p, g) in scaled.items():
        np.testing.assert_array_equal(z[f"mae_{name}_pred"], p)
        np.testing.assert_array_equal(z[f"mae_{name}_gt"], g)
    assert os.path.getsize(MR.GOLDEN) < 100_000


@pytest.mark.parametrize("name", ["scaled_a", "scaled_b", "unit_range"])
def test_compute_mae_restatement_matches_the_recorded_reference(name):
    """compute_mae's data-dependent rescale (max > 1: / 255 and / 65535) and its mean over the map."""
    z = _golden()
    p, g, out = z[f"mae_{name}_pred"][0], z[f"mae_{name}_gt"][0], float(z[f"mae_{name}_out"])
    dp, dg = (255.0 if p.max() > 1.0 else 1.0), (65535.0 if g.max() > 1.0 else 1.0)
    assert (dp, dg) == ((1.0, 1.0) if name == "unit_range" else (255.0, 65535.0))
    ang, bound, _ = MR.angular_error_reference(p, g, pred_divisor=dp, gt_divisor=dg)
    s, valid, invalid, b = MR.angle_sum_reference(ang, bound)
    assert invalid == 0
    # torch's float32 mean: the sum's bound over the count, plus the division's and the result's own rounding
    assert abs(out - s / valid) <= b / valid + 2 * MR.U * s / valid


def test_an_angle_just_outside_its_bound_is_rejected():
    p, g = MR.normal_pair("random", 7, 5, 3)
    ang, bound, _ = MR.angular_error_reference(p, g)
    LBcheck(ang + 0.99 * bound, ang, bound, "inside")
    with pytest.raises(AssertionError):
        LBcheck(ang + 1.01 * bound * (np.arange(35).reshape(7, 5) == 17), ang, bound, "outside")
    # the bound carries acos's conditioning: a nearly parallel pair is allowed more than a perpendicular one (float32 cosines near 1 resolve no angle below 0.03 degrees), but not a tenth of a degree
    near = np.array([[[1.0]], [[1e-4]], [[0.0]]], np.float32)
    ex = np.array([[[1.0]], [[0.0]], [[0.0]]], np.float32)
    ey = np.array([[[0.0]], [[1.0]], [[0.0]]], np.float32)
    b_near, b_perp = MR.angular_error_reference(near, ex)[1][0, 0], MR.angular_error_reference(ey, ex)[1][0, 0]
    assert b_perp < 1e-4 < b_near < 0.1


# ------------------------------------------------------------------------------------------------------------ quantiser
def test_quantiser_restatement_equals_the_torch_float32_chain_bit_for_bit():
    e = MR.quantizer_edge_values()
    assert e.size == 5 * 511
    extra = np.array([-1.0, -1e-8, 0.0, 1.0, 1.0 + 1e-6, 2.0, 300.0], np.float32)
    t = np.concatenate([e, extra])
    want = torch.from_numpy(t).mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
    np.testing.assert_array_equal(MR.quantize_levels(t), want.numpy())
    back = want.to(torch.float32).div(255).numpy()
    got = MR.quantize8(t)
    np.testing.assert_array_equal(got.astype(np.float32).view(np.uint32), back.view(np.uint32))
    assert (got == got.astype(np.float32)).all()
    # On this set a contracted quantiser gives the same levels: t * 255 + 0.5 rounded once and rounded twice truncate alike at every
    # threshold (also at +-64 ulp around each, searched when this test was written).  Equality with torch therefore holds the kernel's
    # levels, not its instruction choice; where contraction does move values (by an ulp) is the compositing step in front of it:
    fused = np.floor(np.clip((t.astype(np.float64) * 255.0 + 0.5).astype(np.float32), 0, 255)).astype(np.uint8)
    np.testing.assert_array_equal(fused, want.numpy())
    shape = (3, 33, 31)
    v, g = MR.image_pair("uniform", shape, 5)
    kw = MR.presentation_inputs("clamp_composite_quantize", shape, 5)
    a = np.clip(kw["alpha"].astype(np.float64), 0, 1)[None]
    bg = kw["background"].astype(np.float64).reshape(3, 1, 1)
    v64 = np.clip(v.astype(np.float64), 0, 1)
    contracted = MR.f32(v64 * a + MR.f32(MR.f32(1.0 - a) * bg))          # fma(v, a, (1 - a) * bg): one rounding less
    separate = MR.composite(v64, a[0], kw["background"])
    assert (contracted != separate).any()


def test_composite_edge_cases_tell_a_fused_multiply_add_apart():
    """At every COMPOSITE_EDGES pixel the restatement equals torch, and the contracted form it was found for gives another 8-bit level:
    the GPU test on this image fails if the kernel's composite loses one of its separate roundings."""
    img, alpha, bg = MR.composite_edge_image()
    kw = dict(alpha=alpha, background=bg, quantize=True)
    v, _, lv, _ = MR.present(img, img, **kw)
    tv, _, tlv, _ = MR.torch_present(img, img, **kw)
    np.testing.assert_array_equal(v.astype(np.float32), tv)
    np.testing.assert_array_equal(lv, tlv)
    t64, a64 = img.astype(np.float64), alpha.astype(np.float64)
    for i, (_, _, c) in enumerate(MR.COMPOSITE_EDGES):
        which = 0 if i < 4 else 1
        other = MR.quantize_levels(MR.composite_contracted(t64, a64, bg, which))
        assert other[c, i // 4, i % 4] != tlv[c, i // 4, i % 4], i


@pytest.mark.parametrize("variant", MR.VARIANTS)
def test_presentation_restatement_equals_the_torch_float32_chain(variant):
    shape = (3, 33, 31)
    for family in ("uniform", "out_of_range", "quantizer_edges"):
        v, g = MR.image_pair(family, shape, 5)
        kw = MR.presentation_inputs(variant, shape, 5)
        a, b, la, lb = MR.present(v, g, **kw)
        ta, tb, tla, tlb = MR.torch_present(v, g, **kw)
        np.testing.assert_array_equal(a.astype(np.float32), ta)
        np.testing.assert_array_equal(b.astype(np.float32), tb)
        if kw.get("quantize"):
            np.testing.assert_array_equal(la, tla)
            np.testing.assert_array_equal(lb, tlb)
        else:
            assert la is None and tla is None


# ---------------------------------------------------------------------------------------------------------- psnr and mse
def test_psnr_and_mse_known_answers(hip_lib_built):
    """mse = mean of squared differences per image, psnr = 20 log10(1 / sqrt(mse)): a constant difference of 0.1 is 20 dB, of 0.5 is
    6.0206 dB, one pixel of 12 off by 1 is 10 log10(12) dB; identical images give inf.  (Host tensors: the torch expression; the
    device path is held to the same answers in tests/test_gpu_metrics.py.)"""
    from utils.image_utils import mse, psnr, psnr_map
    a = torch.zeros(3, 1, 3, 4)
    b = a.clone()
    b[0] += 0.1
    b[1] += 0.5
    b[2, 0, 0, 0] = 1.0
    m, p = mse(a, b), psnr(a, b)
    assert m.shape == (3, 1) and p.shape == (3, 1)
    np.testing.assert_allclose(m[:, 0].numpy(), [0.01, 0.25, 1.0 / 12.0], rtol=1e-6)
    np.testing.assert_allclose(p[:, 0].numpy(), [20.0, 20.0 * math.log10(2.0), 10.0 * math.log10(12.0)], rtol=1e-5)
    assert torch.isinf(psnr(a, a)).all() and (psnr(a, a) > 0).all()
    pm = psnr_map(a, b)
    assert pm.shape == (3, 1, 3, 4) and abs(float(pm[0, 0, 0, 0]) - 20.0) < 1e-4
    # with a gradient required the result is differentiable: d mse / d a = 2 (a - b) / n
    x = a.clone().requires_grad_(True)
    mse(x, b).sum().backward()
    np.testing.assert_allclose(x.grad[1].numpy(), np.full((1, 3, 4), 2 * -0.5 / 12.0), rtol=1e-6)
    assert MR.psnr(0.12, 12) == pytest.approx(20.0) and MR.psnr(0.0, 12) == float("inf")


def test_sum_bounds_reject_an_error_just_outside(hip_lib_built):
    v, g = MR.image_pair("uniform", (3, 33, 31), 9)
    ref, bnd = MR.image_sums_reference(v.astype(np.float64), g.astype(np.float64))
    for k in ("sse", "sad", "ssim"):
        assert 0 < bnd[k] < 1e-4 * abs(ref[k])
        MR.check_scalar(ref[k] + 0.99 * bnd[k], ref[k], bnd[k], k)
        with pytest.raises(AssertionError):
            MR.check_scalar(ref[k] - 1.01 * bnd[k], ref[k], bnd[k], k)
    # known answers of the sums themselves
    c1, c2 = MR.image_pair("constants", (1, 5, 7), 0)
    r, _ = MR.image_sums_reference(c1.astype(np.float64), c2.astype(np.float64))
    d = float(np.float32(0.3)) - float(np.float32(0.7))
    assert r["sse"] == pytest.approx(35 * d * d, rel=1e-12) and r["sad"] == pytest.approx(35 * abs(d), rel=1e-12)
    i1, i2 = MR.image_pair("identical", (3, 5, 7), 0)
    r, b = MR.image_sums_reference(i1.astype(np.float64), i2.astype(np.float64))
    assert r["sse"] == 0.0 and b["sse"] == 0.0 and r["ssim"] == pytest.approx(105.0, abs=1e-9)


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr_hip.h")).read(), flags=re.S)


V, Z, I, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float


@pytest.mark.parametrize("name, ret, args", [
    ("gsr_image_metrics_scratch_floats", "size_t", [I, I, I]),
    ("gsr_image_metrics", "int", [V, V, I, I, I, I, V, V, V, V, V, Z, V, V, V]),
    ("gsr_normal_mae_scratch_floats", "size_t", [I, I]),
    ("gsr_normal_mae", "int", [V, V, I, I, F, F, F, V, V, Z, V, V]),
])
def test_metric_entries_are_declared_exported_and_bound(hip_lib_built, name, ret, args):
    import _gsr
    m = re.search(r"(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, _header(), flags=re.S)
    assert m and m.group(1) == ret, f"{name} is not declared in gsr_hip.h"
    assert hasattr(ctypes.CDLL(_gsr.LIB_PATH), name)
    assert name in _gsr.EXPORTED
    fn = getattr(_gsr.lib, name)
    assert list(fn.argtypes) == args
    assert fn.restype == (ctypes.c_size_t if ret == "size_t" else ctypes.c_int)
    assert _gsr.lib.gsr_version() == 102          # added without an ABI version change


def test_scratch_sizes(hip_lib_built):
    import _gsr
    f, h = _gsr.lib.gsr_image_metrics_scratch_floats, _gsr.lib.gsr_normal_mae_scratch_floats
    assert f(0, 4, 4) == 0 and f(3, -1, 4) == 0 and f(3, 4, 0) == 0 and h(0, 5) == 0 and h(5, -1) == 0
    assert f(3, 32, 32) == 12 and f(3, 33, 31) == 24 and f(3, 1080, 1920) == 4 * 3 * 34 * 60
    assert h(1, 1) == 4 and h(1080, 1920) == 4096


def _image_args(**over):
    import _gsr
    a = dict(img=FAKE, gt=FAKE, C=3, H=33, W=31, flags=3, alpha=None, mask=None, bg=None, row=FAKE, scratch=FAKE,
             nfloats=_gsr.lib.gsr_image_metrics_scratch_floats(3, 33, 31), img_u8=None, gt_u8=None, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("case, over, expect", [
    ("img", dict(img=None), "NULL"), ("gt", dict(gt=None), "NULL"), ("row", dict(row=None), "NULL"),
    ("C", dict(C=0), "invalid size"), ("H", dict(H=-3), "invalid size"), ("W", dict(W=0), "invalid size"),
    ("u8_img", dict(flags=1, img_u8=FAKE), "GSR_PRESENT_QUANT8"), ("u8_gt", dict(flags=0, gt_u8=FAKE), "GSR_PRESENT_QUANT8"),
    ("alpha_no_bg", dict(alpha=FAKE), "background"), ("mask_no_bg", dict(mask=FAKE), "background"),
    ("scratch_null", dict(scratch=None), "scratch"), ("scratch_small", dict(nfloats=23), "scratch"),
    ("scratch_misaligned", dict(scratch=FAKE + 4), "16-byte aligned"), ("flags", dict(flags=4), "flags"),
])
def test_image_metrics_refuses_bad_arguments_before_any_device_call(hip_lib_built, case, over, expect):
    import _gsr
    rc = _gsr.lib.gsr_image_metrics(*_image_args(**over))
    msg = _gsr.lib.gsr_last_error().decode()
    assert rc == GSR_E_INVALID, (case, rc, msg)
    assert msg.startswith("gsr_image_metrics:") and expect in msg, (case, msg)


@pytest.mark.parametrize("case, over, expect", [
    ("pred", dict(pred=None), "NULL"), ("gt", dict(gt=None), "NULL"), ("row", dict(row=None), "NULL"),
    ("H", dict(H=0), "invalid size"), ("W", dict(W=-1), "invalid size"), ("divisor", dict(dp=0.0), "divisors"),
    ("scratch_null", dict(scratch=None), "scratch"), ("scratch_small", dict(nfloats=3), "scratch"),
    ("scratch_misaligned", dict(scratch=FAKE + 8), "16-byte aligned"),
])
def test_normal_mae_refuses_bad_arguments_before_any_device_call(hip_lib_built, case, over, expect):
    import _gsr
    a = dict(pred=FAKE, gt=FAKE, H=7, W=5, dp=1.0, dg=1.0, eps=1e-8, row=FAKE, scratch=FAKE, nfloats=_gsr.lib.gsr_normal_mae_scratch_floats(7, 5),
             emap=None, stream=None)
    a.update(over)
    rc = _gsr.lib.gsr_normal_mae(*a.values())
    msg = _gsr.lib.gsr_last_error().decode()
    assert rc == GSR_E_INVALID, (case, rc, msg)
    assert msg.startswith("gsr_normal_mae:") and expect in msg, (case, msg)


def test_python_layer_validates_before_the_device(hip_lib_built):
    import gsr_eval
    from utils import mae_utils
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mae_utils.angular_error_map(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="batch size"):
        mae_utils.compute_mae(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="4D"):
        mae_utils.compute_mae(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    assert gsr_eval.psnr_from_sums(0.12, 12) == pytest.approx(20.0) and np.isinf(gsr_eval.psnr_from_sums(0.0, 12))
    assert np.isnan(gsr_eval.mae_from_sums(10.0, 4, 1)) and gsr_eval.mae_from_sums(10.0, 4, 0) == 2.5
    assert "LPIPS" in gsr_eval.__doc__ and "LPIPS" in gsr_eval.evaluate_views.__doc__
