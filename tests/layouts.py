"""Layout variants of a tensor: the views a caller of the Python surface sends instead of a fresh contiguous tensor.

Every binding of the package turns a tensor into a raw pointer.  A binding that forgets `.contiguous()`, views where it had to reshape, or
takes `empty_like` of a strided tensor computes on the wrong elements without any error.  `variants_of(base)` returns views with the
shape, dtype and VALUES of `base` (torch.equal holds) whose memory is laid out differently:

    transposed     a permuted parent: the first dimension is the parent's last (a [C,H,W] image made from an HWC array, a matrix that is
                   the `.transpose(0, 1)` of another)
    column_slice   columns [2, 2 + cols) of a row-major parent that is five columns wider (means3D = flat[:, 2:5])
    offset         a contiguous view one element into its storage: the pointer is not a multiple of 16 bytes
    strided_rows   every second row of a parent with twice the rows
    expanded       a stride-0 expansion of the first row (only for a base whose rows are all equal: constants, the gradient of sum())

What the parents guarantee:
  * the variant's values never sit where a layout-blind read would look for them: every other element of a parent is SENTINEL (1e3,
    finite on purpose: a blind read gives a clearly wrong finite result, not NaN that a comparison could mistake for "both NaN");
  * every parent has FULL-SIZE backing storage: from the variant's first element to the end of the storage there are at least
    `numel` elements (from the storage's start, for `offset`).  A layout-blind kernel therefore reads wrong values, never memory outside
    the allocation.  The one exception is `expanded`, whose storage is a single row by construction; tests/test_layouts_host.py checks
    there that `.contiguous()` materialises every element instead.

`blind_read(view)` is that layout-blind read, computed with as_strided on the parent's storage: the negative control that shows a value
comparison would notice a binding that ignores strides (or, for `offset`, the storage offset).  Not a conftest: tests import it.
"""
import torch

SENTINEL = 1e3
KINDS = ("transposed", "column_slice", "offset", "strided_rows", "expanded")


def _fill_value(dtype):
    return True if dtype == torch.bool else SENTINEL


def _full(shape, like):
    return torch.full(shape, _fill_value(like.dtype), dtype=like.dtype, device=like.device)


def transposed(base):
    parent = base.movedim(0, -1).contiguous()
    return parent.movedim(-1, 0)


def column_slice(base):
    rows = base.shape[0]
    cols = base.numel() // rows
    parent = _full((rows, cols + 5), base)
    parent[:, 2:2 + cols] = base.reshape(rows, cols)
    view = parent[:, 2:2 + cols]
    if base.dim() == 1:
        return view[:, 0]
    return view.unflatten(1, tuple(base.shape[1:])) if base.dim() > 2 else view


def offset(base):
    n = base.numel()
    parent = _full((n + 9,), base)
    parent[1:1 + n] = base.reshape(-1)
    return parent[1:1 + n].view(base.shape)


def strided_rows(base):
    parent = _full((2 * base.shape[0],) + tuple(base.shape[1:]), base)
    parent[1::2] = base
    return parent[1::2]


def expanded(base):
    return base[0:1].clone().expand(base.shape)


_MAKERS = dict(transposed=transposed, column_slice=column_slice, offset=offset, strided_rows=strided_rows, expanded=expanded)


def applicable(base, kind):
    """Whether `kind` gives a different layout of `base` with the same values."""
    if base.numel() == 0 or base.dim() == 0 or not base.is_contiguous():
        return False
    if base.dim() > 1 and base.shape[0] == 1:       # a [1,H,W] plane: lay out the [H,W] image, put the leading 1 back
        return applicable(base[0], kind)
    if kind == "offset":
        return base.element_size() % 16 != 0
    if kind == "expanded":
        return base.shape[0] > 1 and bool((base == base[0:1]).all())
    if kind == "transposed":
        return base.dim() >= 2 and base.shape[0] > 1 and base.numel() > base.shape[0]
    return base.shape[0] > 1            # column_slice, strided_rows


def variant(base, kind):
    if not applicable(base, kind):
        raise ValueError(f"layout {kind!r} does not apply to a tensor of shape {tuple(base.shape)}")
    v = variant(base[0], kind)[None] if (base.dim() > 1 and base.shape[0] == 1) else _MAKERS[kind](base)
    assert v.shape == base.shape and v.dtype == base.dtype and v.device == base.device
    return v


def variants_of(base, kinds=KINDS):
    """{kind: view} for every kind of `kinds` that applies to `base` (a contiguous tensor)."""
    return {k: variant(base, k) for k in kinds if applicable(base, k)}


def is_laid_out_differently(view):
    """Non-contiguous, or (a contiguous view at an offset) a pointer that is not 16-byte aligned."""
    return (not view.is_contiguous()) or view.data_ptr() % 16 != 0


def storage_elements(view):
    return view.untyped_storage().nbytes() // view.element_size()


def _storage_flat(view):
    return torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage(), 0, (storage_elements(view),), (1,))


def blind_read(view, ignore_offset=False):
    """What a binding reads that takes `numel` row-major elements at the view's first element (ignore_offset: at the start of its storage,
    as one that drops the storage offset does).  None where the storage is shorter than that (`expanded`)."""
    start = 0 if ignore_offset else view.storage_offset()
    if start + view.numel() > storage_elements(view):
        return None
    strides = []
    step = 1
    for s in reversed(view.shape):
        strides.append(step)
        step *= s
    return torch.as_strided(_storage_flat(view), tuple(view.shape), tuple(reversed(strides)), start).clone()
