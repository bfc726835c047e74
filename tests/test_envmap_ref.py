"""tests/envmap_ref.py pinned on the CPU: the float64 restatement of gsr_envmap_resize against torch's bicubic interpolation
(align_corners=True) on float64 tensors, the restatement of gsr_envmap_sharpen against this project's _adjust_sharpness between sigmoid and
inverse_sigmoid, and a few known answers.  The GPU tests (tests/test_gpu_envmap.py) rest on the restatement; this file needs no GPU."""
import numpy as np
import pytest
import torch

import envmap_ref as E

RESIZE_PAIRS = [(1, 2), (2, 4), (3, 6), (4, 8), (5, 9), (8, 16), (7, 3), (6, 6), (4, 1)]
SHARPEN_SIZES = [1, 2, 3, 4, 5, 17]
FACTORS = [0.0, 1.0, 2.0]
# A weight is a degree-3 Horner form whose intermediates reach 6: three multiply-add steps of at most 2 roundings, each at most
# 6 * 2^-53, so 18 * 2^-52 per weight at the worst and 72 * 2^-52 for the sum of four.
WEIGHT_SUM_ERR = 72 * 2.0 ** -52


def _texture(L, seed, span=1.0):
    return (torch.rand(6, 3, L, L, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * span


@pytest.mark.parametrize("L_src, L_dst", RESIZE_PAIRS)
def test_resize_restatement_is_torch_bicubic_align_corners(L_src, L_dst):
    src = _texture(L_src, 100 * L_src + L_dst)
    want = torch.nn.functional.interpolate(src, size=(L_dst, L_dst), mode="bicubic", align_corners=True).numpy()
    got = E.resize(src.numpy(), L_dst)
    assert got.shape == want.shape == (6, 3, L_dst, L_dst)
    err = float(np.abs(got - want).max())
    print(f"resize {L_src} -> {L_dst}: max |restatement - torch float64| = {err:.3e}")
    assert err <= 1e-13


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("L", SHARPEN_SIZES)
def test_sharpen_restatement_is_the_encoders_filter(hip_lib_built, L, factor):
    from cubemapencoder.cubemap_encoder import _adjust_sharpness      # (the module binds the built library at import)
    x = _texture(L, 7 * L + int(factor), span=9.0)       # [-9, 9]: sigmoid reaches below 1e-3 and above 1 - 1e-3
    x.view(-1)[0], x.view(-1)[-1] = -9.0, 9.0
    s = _adjust_sharpness(torch.sigmoid(x), factor).clamp(min=1e-3, max=1 - 1e-3)
    want = torch.log(s / (1 - s)).numpy()
    got = E.sharpen(x.numpy(), factor)
    act = E.sharpen_activated(x.numpy(), factor)
    assert act.min() == E.LO and act.max() == E.HI       # both clamps are reached
    err = float(np.abs(got - want).max())
    print(f"sharpen L = {L}, factor = {factor}: max |restatement - torch float64| = {err:.3e}")
    # the only difference is the order of the 10-term sum (conv2d with weights 1/13 and 5/13): a few ulp of a value in [0, 1], seen
    # through the logit's slope 1 / (o (1 - o)) <= 1001 at the clamps
    assert err <= 1e-11


def test_known_weights():
    assert E.cubic_weights(0.5).tolist() == [-0.09375, 0.59375, 0.59375, -0.09375]
    assert E.cubic_weights(0.0).tolist() == [0.0, 1.0, 0.0, 0.0]
    t = np.linspace(0.0, 1.0, 257)
    assert np.abs(E.cubic_weights(t).sum(-1) - 1.0).max() <= WEIGHT_SUM_ERR       # a partition of unity


def test_source_coords_come_from_integers():
    i, t = E.source_coords(5, 9)
    assert i.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4] and t.tolist() == [0, 0.5] * 4 + [0]
    i, t = E.source_coords(4, 1)
    assert i.tolist() == [0] and t.tolist() == [0.0]
    i, t = E.source_coords(1, 2)
    assert i.tolist() == [0, 0] and t.tolist() == [0.0, 0.0]
    i, t = E.source_coords(128, 256)
    assert i[-1] == 127 and t[-1] == 0.0 and i[0] == 0 and t[0] == 0.0 and (t[1:-1] > 0).all()


def test_resize_reproduces_coinciding_nodes_exactly():
    src = _texture(5, 3).numpy()
    assert np.array_equal(E.resize(src, 5), src)
    assert np.array_equal(E.resize(src, 9)[..., ::2, ::2], src)
    for L_dst in (1, 2, 3, 10):
        out = E.resize(src, L_dst)
        assert np.array_equal(out[..., 0, 0], src[..., 0, 0])
        if L_dst > 1:
            assert np.array_equal(out[..., [0, 0, -1, -1], [0, -1, 0, -1]], src[..., [0, 0, -1, -1], [0, -1, 0, -1]])


def test_factor_one_leaves_the_sigmoid_unchanged_away_from_the_clamps():
    x = _texture(6, 11, span=3.0).numpy()                # |x| <= 3: sigmoid in [0.047, 0.953]
    assert np.abs(E.sharpen_activated(x, 1.0) - E.sigmoid(x)).max() == 0.0
    assert np.abs(E.sharpen(x, 1.0) - x).max() <= 1e-14


@pytest.mark.parametrize("value", [-2.5, 0.0, 0.75])
def test_a_constant_plane_stays_constant(value):
    src = np.full((6, 3, 5, 5), value)
    for L_dst in (1, 3, 5, 10):
        # value * (sum of the weights along x) * (sum along y), plus the roundings of the two 4-term sums themselves
        assert np.abs(E.resize(src, L_dst) - value).max() <= (2 * WEIGHT_SUM_ERR + 16 * 2.0 ** -52) * abs(value)
    for factor in FACTORS:
        assert np.abs(E.sharpen(src, factor) - value).max() <= 1e-14
