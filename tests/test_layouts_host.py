"""tests/layouts.py on the host: every variant has the base's values, is really laid out differently, and would be NOTICED — a read that
ignores its strides (or its storage offset) differs from the base in most elements and stays inside the parent's storage.  This is the
negative control of tests/test_gpu_layouts.py: without it, a value comparison that passes would say nothing."""
import pytest
import torch

import layouts

# the shapes the GPU tests lay out: per-Gaussian parameters, SH coefficients with rows that are no multiple of 16 bytes, camera matrices
# and vectors, images, a cubemap, a bool mask
SHAPES = {"means3D": (2003, 3), "shs": (2003, 9, 3), "opacities": (2003, 1), "matrix": (4, 4), "bg": (3,), "image": (3, 120, 200),
          "plane": (1, 120, 200), "cubemap": (6, 3, 16, 16), "ragged": (8, 203, 301)}


# a single column, or a vector, has nothing to transpose (a [1,H,W] plane is laid out as its [H,W] image)
NOT_APPLICABLE = {("opacities", "transposed"), ("bg", "transposed")}


def _base(shape, dtype=torch.float32, constant=False):
    g = torch.Generator().manual_seed(sum(shape))
    t = torch.randn(shape, generator=g)
    if constant:
        t = (t[:, 0:1] if shape[0] == 1 else t[0:1]).expand(shape).contiguous()
    return (t > 0) if dtype == torch.bool else t.to(dtype)


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("kind", [k for k in layouts.KINDS if k != "expanded"])
def test_variant_is_equal_different_and_detectable(name, kind):
    base = _base(SHAPES[name])
    if not layouts.applicable(base, kind):
        assert (name, kind) in NOT_APPLICABLE, (name, kind)
        with pytest.raises(ValueError):
            layouts.variant(base, kind)
        return
    before = base.clone()
    v = layouts.variant(base, kind)
    assert torch.equal(base, before)                      # the base is left alone
    assert v.shape == base.shape and v.dtype == base.dtype
    assert torch.equal(v, base)
    assert layouts.is_laid_out_differently(v)
    if kind == "offset":
        assert v.is_contiguous() and v.data_ptr() % 16 != 0 and v.storage_offset() != 0
        blind = layouts.blind_read(v, ignore_offset=True)        # a binding that drops the storage offset
    else:
        assert not v.is_contiguous()
        blind = layouts.blind_read(v)
    assert blind is not None, "full-size backing storage: the blind read stays inside the parent"
    assert blind.shape == base.shape and bool(torch.isfinite(blind).all())
    assert float((blind != base).float().mean()) > 0.5, (name, kind)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_shape_has_at_least_two_layouts(name):
    assert len(layouts.variants_of(_base(SHAPES[name]))) >= 2, name


def test_every_parent_but_the_expanded_one_is_full_size():
    for name, shape in SHAPES.items():
        for kind, v in layouts.variants_of(_base(shape)).items():
            start = 0 if kind == "offset" else v.storage_offset()
            assert layouts.storage_elements(v) - start >= v.numel(), (name, kind)


@pytest.mark.parametrize("name", ["opacities", "image", "plane", "means3D"])
def test_expanded(name):
    shape = SHAPES[name]
    base = _base(shape, constant=True)
    v = layouts.variant(base, "expanded")
    assert torch.equal(v, base) and not v.is_contiguous() and 0 in v.stride()
    assert layouts.storage_elements(v) < v.numel() and layouts.blind_read(v) is None      # one row of storage: nothing to read blindly
    c = v.contiguous()
    assert c.is_contiguous() and layouts.storage_elements(c) >= base.numel() and torch.equal(c, base)      # every element materialised
    assert not layouts.applicable(_base(shape), "expanded")          # rows differ: not a constant


def test_bool_masks_and_sentinels():
    base = _base((2003,), torch.bool)
    for kind, v in layouts.variants_of(base).items():
        assert v.dtype == torch.bool and torch.equal(v, base) and layouts.is_laid_out_differently(v), kind
    base = _base((2003, 3))
    for kind in ("column_slice", "strided_rows", "offset"):
        v = layouts.variant(base, kind)
        flat = layouts._storage_flat(v)
        rest = int((flat == layouts.SENTINEL).sum())
        assert rest == flat.numel() - base.numel(), kind          # everything that is not the variant is the finite sentinel
    assert float(base.abs().max()) < layouts.SENTINEL / 100


def test_views_of_non_contiguous_or_empty_bases_are_refused():
    base = _base((6, 4))
    for bad in (base.t(), base[:0], torch.tensor(1.0)):
        for kind in layouts.KINDS:
            assert not layouts.applicable(bad, kind)
