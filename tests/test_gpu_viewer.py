"""The viewer presentation kernels (csrc/gsr_viewer.hip) and their Python layer (utils/image_utils.py) on the GPU against
tests/viewer_ref.py: every mode at the shapes where a four-pixel lane, a 64-lane row and a halo tile go wrong, bit for bit against
torch's float32 chain on the CPU where the order of operations is fixed, and against the float64 gradient within its bound where it
is not."""
import numpy as np
import pytest
import torch

import loss_bounds as LB
import viewer_ref as VR

pytestmark = pytest.mark.gpu

N_MODES = len(VR.ITEMS)
_refs = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(family, H, W, seed=11):
    """(rgb_out, package) as numpy and on the device, and per mode the torch chain's result: computed once, never modified."""
    key = (family, H, W, seed)
    if key not in _refs:
        rgb, pkg = VR.package(family, H, W, seed)
        table = VR.turbo()
        chains = {m: VR.torch_chain(rgb, pkg, VR.ITEMS, m, table) for m in range(N_MODES) if VR.defined(family, VR.ITEMS, m, H, W)}
        _refs[key] = (rgb, pkg, _dev(rgb), {k: _dev(v) for k, v in pkg.items()}, chains)
    return _refs[key]


def _ramp():
    """A table whose row i is (i, i, i): the colour-mapped image is the index plane."""
    return torch.arange(256, dtype=torch.float32, device="cuda")[:, None].repeat(1, 3).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_mode(family, H, W, mode):
    from utils import image_utils as IU
    rgb, pkg, drgb, dpkg, chains = _case(family, H, W)
    img, frame, idx, grad = chains[mode]
    name = f"{family} {VR.ITEMS[mode]} {H}x{W}"
    got_f = IU.render_net_image(drgb, dpkg, VR.ITEMS, mode, None)
    got_b = IU.present_bytes(drgb, dpkg, VR.ITEMS, mode)
    assert got_f.shape == (3, H, W) and got_f.dtype == torch.float32 and got_b.shape == (H, W, 3) and got_b.dtype == torch.uint8
    assert got_b.is_contiguous() and got_b.is_cuda
    src, half, sobel, repeated = VR.select(rgb, pkg, VR.ITEMS, mode)
    if not sobel:
        np.testing.assert_array_equal(got_b.cpu().numpy(), frame, err_msg=f"{name}: frame")
        np.testing.assert_array_equal(_bits(got_f.cpu().numpy()), _bits(img), err_msg=f"{name}: float image")
        if idx is not None:
            got_idx = IU.colormap(dpkg[VR.MODES[VR.ITEMS[mode].lower()][0]], cmap=_ramp())[0].cpu().numpy()
            np.testing.assert_array_equal(got_idx, idx, err_msg=f"{name}: colour index")
        return
    # curvature: the gradient within its bound, the index the float64 index or one level off near a rounding boundary, and the
    # image and frame the table at the kernel's own index
    table = VR.turbo()
    r = VR.restate(rgb, pkg, VR.ITEMS, mode, table)
    g = IU.gradient_map(_dev(((src + np.float32(1)) / np.float32(2)).astype(np.float32))).cpu().numpy()
    q = LB.check(g, r["grad"], r["bound"], what=f"{name}: gradient")
    got_idx = IU._present(dpkg["rend_normal"], 1 | 2 | 4, cmap=_ramp())[0][0].cpu().numpy().astype(np.int64)
    share = VR.check_indices(got_idx, r["idx"], r["near"], name)
    print(f"measured {name}: gradient error {q:.3f} of the bound, {share:.5f} of the pixels one level off")
    np.testing.assert_array_equal(_bits(got_f.cpu().numpy()), _bits(table[got_idx].transpose(2, 0, 1)), err_msg=f"{name}: float image")
    np.testing.assert_array_equal(got_b.cpu().numpy(), VR.frame_bytes(table[got_idx].transpose(2, 0, 1)), err_msg=f"{name}: frame")
    if got_idx.max() > 0:
        assert got_idx.max() == 255 and got_idx.min() == 0          # the pixels that define max and min map to the ends exactly


@pytest.mark.parametrize("mode", range(N_MODES), ids=[m.replace(" ", "_") for m in VR.ITEMS])
def test_every_mode_at_the_edge_shapes(mode):
    for H, W in VR.SHAPES:
        for family in VR.FAMILIES:
            if VR.defined(family, VR.ITEMS, mode, H, W):
                check_mode(family, H, W, mode)


def test_full_size():
    """1080 x 1920, every mode on noisy unit normals / smooth maps."""
    H, W = VR.FULL_SIZE
    for mode in range(N_MODES):
        check_mode("normals", H, W, mode)


def test_gradient_map_one_and_three_channels():
    from utils import image_utils as IU
    for (H, W) in VR.SOBEL_SHAPES + ((1, 1), (1, 7), (7, 1)):
        for C in (1, 3):
            for family in ("smooth", "normals", "out_of_range"):
                x = VR.image(family, C, H, W, 31)
                ref, bound = VR.gradient_reference(x, half=False)
                got = IU.gradient_map(_dev(x))
                assert got.shape == (1, H, W)
                q = LB.check(got.cpu().numpy(), ref, bound, what=f"gradient_map {family} C={C} {H}x{W}")
                print(f"measured gradient_map {family} C={C} {H}x{W}: {q:.3f} of the bound")


def test_zero_padding_comes_after_the_affine():
    """A constant normal image has curvature on the frame's outer ring only: outside the image the padded value is 0, not 0.5."""
    from utils import image_utils as IU
    for H, W in ((33, 31), (64, 65), (17, 130)):
        _, pkg = VR.package("constant", H, W, 2)
        ref, bound = VR.gradient_reference(pkg["rend_normal"], half=True)
        got = IU._present(_dev(pkg["rend_normal"]), 1 | 2)[0].cpu().numpy()
        LB.check(got, ref, bound, what=f"constant normals {H}x{W}")
        inner = np.zeros((H, W), bool)
        inner[1:-1, 1:-1] = True
        assert (np.abs(got[0][inner]) <= bound[0][inner]).all() and (got[0][~inner] > 0.1).all()
        idx = IU._present(_dev(pkg["rend_normal"]), 1 | 2 | 4, cmap=_ramp())[0][0].cpu().numpy()
        assert (idx[inner] == 0).all() and (idx[~inner] > 0).all()


def test_constant_map_gives_index_zero():
    from utils import image_utils as IU
    table = torch.from_numpy(VR.turbo()).cuda()
    for H, W in ((1, 1), (5, 3), (64, 65)):
        m = torch.full((1, H, W), 0.37, device="cuda")
        got = IU.colormap(m)
        assert got.shape == (3, H, W) and torch.equal(got, table[0].reshape(3, 1, 1).expand(3, H, W))
        assert torch.equal(IU.colormap(m[0], cmap=_ramp()), torch.zeros(3, H, W, device="cuda"))
        frame = IU.present_bytes(None, {"rend_alpha": m}, ["Alpha"], 0)
        assert torch.equal(frame, (table[0] * 255).byte().expand(H, W, 3))


def test_a_nan_pixel_gives_byte_zero():
    from utils import image_utils as IU
    for H, W in ((5, 3), (64, 65)):
        rgb, pkg, drgb, dpkg, chains = _case("nan", H, W)
        for mode in chains:
            src = VR.select(rgb, pkg, VR.ITEMS, mode)[0]
            assert np.isnan(src).sum() == 1
            frame = IU.present_bytes(drgb, dpkg, VR.ITEMS, mode).cpu().numpy()
            c, y, x = np.argwhere(np.isnan(src))[0]
            assert (frame[y, x, c] == 0) if src.shape[0] == 3 else (frame[y, x] == 0).all()
            np.testing.assert_array_equal(frame, chains[mode][1])


def test_present_bytes_on_a_render_fast_package():
    """A real package of a small synthetic scene, 64 x 65: present_bytes equals the composed expression for every mode the package
    serves, falls back to mode 0 past the end of the list, raises KeyError where render_fast returns no such map, and fills `out`."""
    from gaussian_renderer import render_fast
    from helpers import S
    from test_gpu_dropin import _Pipe, _model, _scene, _view
    from utils import image_utils as IU
    H, W = 64, 65
    t, env = _scene(3000, 5, -2.0, 16)
    View = _view(S.look_at_camera(W, H, eye=(0.4, -0.3, -1.0), target=(0, 0, 5)), W, H)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    with torch.no_grad():
        pkg = render_fast(View, _model(t, env), _Pipe, bg)
    rgb_out = pkg["render"].clamp(0, 1)
    assert float(pkg["rend_alpha"].max()) > 0.5
    served = 0
    for mode, item in enumerate(VR.ITEMS):
        key = VR.MODES.get(item.lower(), ("render",))[0]
        if key not in pkg:
            with pytest.raises(KeyError):
                IU.present_bytes(rgb_out, pkg, VR.ITEMS, mode)
            with pytest.raises(KeyError):
                IU.render_net_image(rgb_out, pkg, VR.ITEMS, mode, View)
            continue
        net = IU.render_net_image(rgb_out, pkg, VR.ITEMS, mode, View)
        want = (torch.clamp(net, min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous()
        got = IU.present_bytes(rgb_out, pkg, VR.ITEMS, mode)
        assert net.shape == (3, H, W) and torch.equal(got, want), item
        served += 1
    assert served == 8 and "surf_depth" not in pkg          # depth, edge and mask need render()'s surface outputs
    first = IU.present_bytes(rgb_out, pkg, VR.ITEMS, 0)
    assert torch.equal(IU.present_bytes(rgb_out, pkg, VR.ITEMS, N_MODES), first)
    assert torch.equal(IU.present_bytes(rgb_out, pkg, VR.ITEMS, N_MODES + 5), first)
    assert torch.equal(IU.render_net_image(rgb_out, pkg, VR.ITEMS, 99, View), rgb_out)
    out = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda")
    back = IU.present_bytes(rgb_out, pkg, VR.ITEMS, VR.ITEMS.index("Curvature"), out=out)
    assert back is out and torch.equal(out, IU.present_bytes(rgb_out, pkg, VR.ITEMS, VR.ITEMS.index("Curvature")))
    for bad in (torch.empty((H, W, 3), device="cuda"), torch.empty((W, H, 3), dtype=torch.uint8, device="cuda"),
                torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")[:, :, :3], torch.empty((H, W, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out"):
            IU.present_bytes(rgb_out, pkg, VR.ITEMS, 0, out=bad)


def test_bytes_past_the_end_stay_untouched():
    """out_u8 as a view into a larger buffer with sentinels on both sides, for every width class of the four-pixel lane and both
    alignments of the frame's first byte."""
    from utils import image_utils as IU
    for H, W in ((1, 1), (1, 7), (7, 1), (5, 3), (3, 4), (3, 5), (2, 6), (33, 31), (4, 257), (5, 260)):
        rgb, pkg = VR.package("smooth", H, W, 13)
        drgb, dpkg = _dev(rgb), {k: _dev(v) for k, v in pkg.items()}
        n = H * W * 3
        for lead in (16, 17):
            for mode in (0, VR.ITEMS.index("Alpha"), VR.ITEMS.index("Curvature"), VR.ITEMS.index("Mask")):
                buf = torch.full((lead + n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
                out = buf[lead:lead + n].view(H, W, 3)
                IU.present_bytes(drgb, dpkg, VR.ITEMS, mode, out=out)
                assert (buf[:lead] == 0xA5).all() and (buf[lead + n:] == 0xA5).all(), (H, W, lead, mode)
                assert torch.equal(out, IU.present_bytes(drgb, dpkg, VR.ITEMS, mode)), (H, W, lead, mode)
