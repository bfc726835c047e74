"""The viewer presentation on a machine without a GPU: the committed turbo table, the C entries' export, binding and every refusal before
any device work, the Python layer's own refusals, plot_cubemap and to_3ch against their numpy restatements, and the references of
tests/viewer_ref.py against each other: the numpy restatement against torch's float32 chain, the float64 gradient's bound, and the
share of pixels near a rounding boundary on the inputs the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import viewer_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_E_INVALID = -1
FAKE = 0x7f0000000000          # 256-byte aligned, never dereferenced: every call below must fail validation first
HALF, SOBEL, COLORMAP = 1, 2, 4


# ------------------------------------------------------------------------------------------------------------------- table
def test_turbo_table_is_matplotlibs():
    t = VR.turbo()
    assert t.shape == (256, 3) and t.dtype == np.float32 and t.min() >= 0.0 and t.max() <= 1.0
    # the table as recorded from matplotlib (tests/golden/turbo_lut.npy, float32): the text the product reads gives the same bits
    golden = np.load(os.path.join(ROOT, "tests", "golden", "turbo_lut.npy"))
    assert golden.dtype == np.float32 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "turbo_lut.npy")) < 4096
    np.testing.assert_array_equal(t.view(np.uint32), golden.view(np.uint32))
    assert len({tuple(r) for r in t.tolist()}) == 256          # an image equal to the reference's has the reference's indices
    matplotlib = pytest.importorskip("matplotlib")
    want = torch.tensor(matplotlib.colormaps["turbo"].colors)
    assert want.dtype == torch.float32
    np.testing.assert_array_equal(t.view(np.uint32), want.numpy().view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr_hip.h")).read(), flags=re.S)


V, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


@pytest.mark.parametrize("name, ret, args", [
    ("gsr_present_view_scratch_floats", "size_t", [I, I, I, I]),
    ("gsr_present_view", "int", [V, I, I, I, I, V, V, V, V, Z, V]),
])
def test_viewer_entries_are_declared_exported_and_bound(hip_lib_built, name, ret, args):
    import _gsr
    m = re.search(r"(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, _header(), flags=re.S)
    assert m and m.group(1) == ret, f"{name} is not declared in gsr_hip.h"
    assert hasattr(ctypes.CDLL(_gsr.LIB_PATH), name)
    assert name in _gsr.EXPORTED
    fn = getattr(_gsr.lib, name)
    assert list(fn.argtypes) == args
    assert fn.restype == (ctypes.c_size_t if ret == "size_t" else ctypes.c_int)
    assert _gsr.lib.gsr_version() == 102          # added without an ABI version change
    assert (_gsr.GSR_VIEW_HALF, _gsr.GSR_VIEW_SOBEL, _gsr.GSR_VIEW_COLORMAP) == (HALF, SOBEL, COLORMAP)
    for flag, value in (("GSR_VIEW_HALF", 1), ("GSR_VIEW_SOBEL", 2), ("GSR_VIEW_COLORMAP", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), _header())


def test_scratch_sizes(hip_lib_built):
    import _gsr
    f = _gsr.lib.gsr_present_view_scratch_floats
    for flags in (0, COLORMAP, SOBEL | COLORMAP, 7):
        assert f(0, 4, 4, flags) == 0 and f(1, -1, 4, flags) == 0 and f(3, 4, 0, flags) == 0
    assert f(3, 33, 31, 0) == 0 and f(3, 33, 31, HALF | SOBEL) == 0          # no colour map: nothing crosses a launch
    assert f(1, 33, 31, COLORMAP) == 4 and f(3, 33, 31, HALF | SOBEL | COLORMAP) == 4 + 33 * 31
    assert f(3, 1080, 1920, SOBEL | COLORMAP) == 4 + 1080 * 1920


def _args(**over):
    import _gsr
    a = dict(src=FAKE, C=1, H=33, W=31, flags=COLORMAP, table=FAKE, out_f32=FAKE, out_u8=FAKE, scratch=FAKE, nfloats=None, stream=None)
    a.update(over)
    if a["nfloats"] is None:
        a["nfloats"] = _gsr.lib.gsr_present_view_scratch_floats(a["C"], a["H"], a["W"], a["flags"] & 7)
    return list(a.values())


@pytest.mark.parametrize("case, over, expect", [
    ("src", dict(src=None), "NULL src"),
    ("outputs", dict(out_f32=None, out_u8=None), "both outputs"),
    ("C0", dict(C=0), "invalid size"), ("H", dict(H=-3), "invalid size"), ("W", dict(W=0), "invalid size"),
    ("C2", dict(C=2, flags=0), "expected 1 or 3"), ("C4", dict(C=4, flags=0), "expected 1 or 3"),
    ("map_on_rgb", dict(C=3, flags=COLORMAP), "one-channel"), ("map_on_rgb_half", dict(C=3, flags=HALF | COLORMAP), "one-channel"),
    ("no_table", dict(table=None), "table"), ("no_table_sobel", dict(C=3, flags=HALF | SOBEL | COLORMAP, table=None), "table"),
    ("flags", dict(flags=8), "flags"), ("flags_high", dict(flags=COLORMAP | 64), "flags"),
    ("scratch_null", dict(scratch=None), "scratch"), ("scratch_small", dict(nfloats=3), "scratch"),
    ("scratch_small_sobel", dict(C=3, flags=SOBEL | COLORMAP, nfloats=4 + 33 * 31 - 1), "scratch"),
    ("scratch_misaligned", dict(scratch=FAKE + 4), "16-byte aligned"),
])
def test_present_view_refuses_bad_arguments_before_any_device_call(hip_lib_built, case, over, expect):
    import _gsr
    rc = _gsr.lib.gsr_present_view(*_args(**over))
    msg = _gsr.lib.gsr_last_error().decode()
    assert rc == GSR_E_INVALID, (case, rc, msg)
    assert msg.startswith("gsr_present_view:") and expect in msg, (case, msg)


# ------------------------------------------------------------------------------------------------------------ Python layer
def test_python_layer_validates_before_the_device(hip_lib_built):
    from utils import image_utils as IU
    rgb, pkg = VR.package("smooth", 5, 3, 1)
    tp = {k: torch.from_numpy(v) for k, v in pkg.items()}
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        IU.gradient_map(torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        IU.colormap(torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        IU.render_net_image(torch.from_numpy(rgb), tp, VR.ITEMS, VR.ITEMS.index("Normal"), None)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        IU.present_bytes(torch.from_numpy(rgb), tp, VR.ITEMS, 0)
    with pytest.raises(NotImplementedError, match="viridis"):
        IU.colormap(torch.zeros(1, 4, 4), cmap="viridis")
    with pytest.raises(KeyError):
        IU.present_bytes(torch.from_numpy(rgb), {}, VR.ITEMS, VR.ITEMS.index("Depth"))
    with pytest.raises(TypeError):
        IU.gradient_map(np.zeros((3, 4, 4), np.float32))
    with pytest.raises(RuntimeError, match="Float"):
        IU.gradient_map(torch.zeros(3, 4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="Float"):
        IU.present_bytes(torch.zeros(3, 4, 4, dtype=torch.float16), {}, ["RGB"], 0)
    for bad in ((2, 4, 4), (1, 3, 4, 4), (4,), (3, 0, 4)):
        with pytest.raises(ValueError, match="C = 1 or 3"):
            IU.gradient_map(torch.zeros(*bad))
    with pytest.raises(ValueError, match=r"\[1, H, W\] or \[H, W\]"):
        IU.colormap(torch.zeros(3, 4, 4))
    assert "not provided" not in IU.__doc__ and "max equals its min" in IU.__doc__ and "NaN" in IU.__doc__


def test_plot_cubemap_and_to_3ch_match_their_restatements(hip_lib_built):
    from utils.image_utils import plot_cubemap, to_3ch
    rs = np.random.RandomState(3)
    for C, h, w in ((3, 4, 4), (1, 2, 2), (3, 2, 5)):
        faces = rs.rand(6, C, h, w).astype(np.float32)
        got = plot_cubemap(torch.from_numpy(faces))
        np.testing.assert_array_equal(got.numpy(), VR.cubemap_cross(faces))
        assert got.shape == (3, 3 * h, 4 * w)
    # the cross by hand: face 3 above face 4 (flipped top to bottom), faces 1 4 0 5 in the middle row, face 2 below face 4
    faces = np.arange(6, dtype=np.float32).reshape(6, 1, 1, 1) * np.ones((6, 3, 2, 2), np.float32)
    faces[3, :, 0, :] = 30.0                                   # its first row must come out as the second
    g = plot_cubemap(torch.from_numpy(faces)).numpy()[0]
    assert g[2:4, :].tolist() == [[1, 1, 4, 4, 0, 0, 5, 5]] * 2
    assert g[0:2, 2:4].tolist() == [[3, 3], [30, 30]] and g[4:6, 2:4].tolist() == [[2, 2], [2, 2]]
    assert g[0:2, 0:2].sum() == 0 and g[0:2, 4:].sum() == 0 and g[4:6, 0:2].sum() == 0 and g[4:6, 4:].sum() == 0
    for shape in ((4, 5), (1, 4, 5), (3, 4, 5), (4, 5, 3), (4, 5, 1), (2, 3, 4, 5), (2, 1, 4, 5), (2, 4, 5, 3), (2, 4, 5, 1), (2, 5, 4, 6)):
        a = rs.rand(*shape).astype(np.float32)
        got = to_3ch(torch.from_numpy(a).requires_grad_(True))
        assert got.dim() == 4 and got.shape[1] == 3 and not got.requires_grad
        np.testing.assert_allclose(got.numpy(), VR.three_channels(a), rtol=1e-6)
    assert to_3ch(None) is None
    with pytest.raises(ValueError):
        to_3ch(torch.zeros(5))


# ------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("family", VR.FAMILIES)
def test_restatement_agrees_with_the_torch_float32_chain(family):
    """Pointwise modes: image and frame bit for bit.  Curvature: torch's gradient within the float64 gradient's bound, its colour
    index the float64 index or one level off near a rounding boundary."""
    import loss_bounds as LB
    table = VR.turbo()
    for H, W in ((5, 3), (33, 31), (7, 1)):
        rgb, pkg = VR.package(family, H, W, 11)
        for mode in range(len(VR.ITEMS) + 1):
            if not VR.defined(family, VR.ITEMS, mode, H, W):
                continue
            r = VR.restate(rgb, pkg, VR.ITEMS, mode, table)
            img, frame, idx, grad = VR.torch_chain(rgb, pkg, VR.ITEMS, mode, table)
            assert img.shape == (3, H, W) and frame.shape == (H, W, 3) and frame.dtype == np.uint8
            if r["exact"]:
                np.testing.assert_array_equal(r["img"].view(np.uint32), img.view(np.uint32), err_msg=f"{family} {VR.ITEMS[mode % len(VR.ITEMS)]}")
                np.testing.assert_array_equal(r["frame"], frame)
                if idx is not None:
                    np.testing.assert_array_equal(r["idx"], idx)
            else:
                q = LB.check(grad, r["grad"], r["bound"], what=f"{family} gradient {H}x{W}")
                assert q <= 1.0
                VR.check_indices(idx, r["idx"], r["near"], f"{family} curvature {H}x{W}")
    assert VR.torch_chain(rgb, pkg, VR.ITEMS, len(VR.ITEMS), table)[1].tolist() == VR.torch_chain(rgb, pkg, VR.ITEMS, 0, table)[1].tolist()


def test_nan_and_constant_are_what_the_product_defines():
    table = VR.turbo()
    rgb, pkg = VR.package("nan", 5, 3, 2)
    assert np.isnan(rgb).sum() == 1
    frame = VR.restate(rgb, pkg, VR.ITEMS, 0, table)["frame"]
    y, x, c = 2, 1, 1
    assert frame[y, x, c] == 0 and VR.torch_chain(rgb, pkg, VR.ITEMS, 0, table)[1][y, x, c] == 0
    rgb, pkg = VR.package("constant", 5, 3, 2)
    r = VR.restate(rgb, pkg, VR.ITEMS, VR.ITEMS.index("Alpha"), table)
    assert (r["idx"] == 0).all() and (r["img"] == table[0].reshape(3, 1, 1)).all()
    # a constant normal image: zero padding AFTER the affine makes the outer ring, and only it, non-zero
    g, b = VR.gradient_reference(pkg["rend_normal"], half=True)
    inner = np.zeros((5, 3), bool)
    inner[1:-1, 1:-1] = True
    assert (g[0][inner] == 0).all() and (g[0][~inner] > 0.1).all() and (b[0] < 1e-5).all()


def test_gradient_bound_rejects_an_error_just_outside():
    import loss_bounds as LB
    x = VR.image("normals", 3, 9, 8, 4)
    g, b = VR.gradient_reference(x, half=True)
    assert (b > 0).all() and (b < 1e-5).all()
    LB.check(g + 0.99 * b, g, b, what="inside")
    with pytest.raises(AssertionError):
        LB.check(g + 1.01 * b * (np.arange(72).reshape(1, 9, 8) == 40), g, b, what="outside")
    idx, near, delta = VR.index_reference(g[0], b[0])
    assert idx.min() == 0 and idx.max() == 255 and (delta < 0.01).all()
    with pytest.raises(AssertionError):
        VR.check_indices(idx + (~near & (np.arange(72).reshape(9, 8) == np.argmax(~near))), idx, near, "far from a boundary")


@pytest.mark.parametrize("shape", VR.SOBEL_SHAPES)
def test_near_boundary_share_of_the_sobel_inputs_is_below_the_cap(shape):
    """The GPU test allows a one-level difference only at pixels near a rounding boundary, and at most NEAR_CAP of the pixels: the
    inputs it uses must leave that room.  (Noisy unit normals: a fraction of a percent of the pixels lie within delta.)"""
    H, W = shape
    for family in ("normals", "smooth", "out_of_range", "two_valued"):
        _, pkg = VR.package(family, H, W, 21)
        g, b = VR.gradient_reference(pkg["rend_normal"], half=True)
        _, near, delta = VR.index_reference(g[0], b[0])
        print(f"measured {family} {H}x{W}: near-boundary share {near.mean():.5f}, largest delta {delta.max():.2e}")
        assert near.mean() < VR.NEAR_CAP
