"""The poison harness itself (tests/poison.py), on the CPU: every patched allocation form yields the pattern for every element type the
package allocates, empty tensors pass through, the counter counts, the originals come back after an exception — and a scan of the package
shows that no allocation form other than the patched ones is in use, so a new wrapper cannot escape the harness unnoticed."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

import poison
from poison import PATTERNS, poisoned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-splatting-reflection_amd")

DTYPES = [torch.float32, torch.int32, torch.uint8, torch.bool, torch.int64]
FORMS = {
    "empty": lambda dt: torch.empty((3, 5), dtype=dt),
    "empty_kw": lambda dt: torch.empty(size=(3, 5), dtype=dt, device="cpu"),
    "empty_like": lambda dt: torch.empty_like(torch.zeros((3, 5), dtype=dt)),
    "new_empty": lambda dt: torch.zeros(2, dtype=dt).new_empty((3, 5)),
    "empty_strided": lambda dt: torch.empty_strided((3, 5), (5, 1), dtype=dt),
    "empty_strided_gaps": lambda dt: torch.empty_strided((3, 5), (8, 1), dtype=dt),
}


def _bytes(t):
    st = t.untyped_storage()
    return np.frombuffer(bytes(st), np.uint8) if st.nbytes() else np.zeros(0, np.uint8)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_each_form_yields_the_pattern(form, dtype, pattern):
    with poisoned(pattern, device_type="cpu") as ps:
        t = FORMS[form](dtype)
        assert ps.count == 1 and ps.bytes == t.untyped_storage().nbytes()
    assert t.dtype == dtype and tuple(t.shape) == (3, 5)
    raw = _bytes(t)
    assert raw.size >= 15 * t.element_size() and (raw == pattern).all()
    if dtype == torch.float32:
        v = t.numpy()
        assert {0x00: (v == 0).all(), 0xFF: np.isnan(v).all(), 0x01: ((v > 2.3e-38) & (v < 2.4e-38)).all()}[pattern]
    if dtype == torch.int32:
        assert (t.numpy() == {0x00: 0, 0xFF: -1, 0x01: 16843009}[pattern]).all()
    if dtype == torch.int64:
        assert (t.numpy() == {0x00: 0, 0xFF: -1, 0x01: 0x0101010101010101}[pattern]).all()


def test_zero_size_and_other_devices_pass_through():
    with poisoned(0xFF, device_type="cpu") as ps:
        for t in (torch.empty(0), torch.empty((4, 0, 3), dtype=torch.int32), torch.empty_like(torch.zeros(0)), torch.zeros(1).new_empty((0,)),
                  torch.empty_strided((0, 2), (2, 1))):
            assert t.numel() == 0
        assert ps.count == 0 and ps.bytes == 0
    with poisoned(0xFF, device_type="cuda") as ps:           # a CPU tensor is none of a cuda scope's business
        torch.empty(7)
        assert ps.count == 0 and ps.bytes == 0


def test_the_counter_counts_tensors_and_bytes():
    with poisoned(0x01, device_type="cpu") as ps:
        torch.empty(10, dtype=torch.float32)
        torch.empty((2, 3), dtype=torch.int64)
        torch.empty_like(torch.zeros(5, dtype=torch.uint8))
        torch.zeros(3).new_empty((4,))
        torch.empty(0)
        assert ps.count == 4 and ps.bytes == 40 + 48 + 5 + 16


def test_zeros_and_full_are_left_alone():
    with poisoned(0xFF, device_type="cpu") as ps:
        z, f = torch.zeros(9), torch.full((9,), 2.5)
        zl, nz = torch.zeros_like(f), f.new_zeros((4,))
        o, nf = torch.ones(3, dtype=torch.int32), f.new_full((2,), 7.0)
        assert ps.count == 0
    assert (z == 0).all() and (f == 2.5).all() and (zl == 0).all() and (nz == 0).all() and (o == 1).all() and (nf == 7.0).all()


def test_the_originals_are_restored_also_after_an_exception():
    before = [getattr(owner, name) for owner, name in poison.PATCHED]
    own = [name in vars(owner) for owner, name in poison.PATCHED]
    with pytest.raises(KeyError):
        with poisoned(0xFF, device_type="cpu"):
            assert all(getattr(owner, name) is not b for (owner, name), b in zip(poison.PATCHED, before))
            raise KeyError("inside")
    assert all(getattr(owner, name) is b for (owner, name), b in zip(poison.PATCHED, before))
    assert [name in vars(owner) for owner, name in poison.PATCHED] == own          # an inherited attribute is inherited again
    with poisoned(0x01, device_type="cpu"):
        pass
    assert all(getattr(owner, name) is b for (owner, name), b in zip(poison.PATCHED, before))
    with pytest.raises(ValueError):
        with poisoned(0x100, device_type="cpu"):
            pass
    assert all(getattr(owner, name) is b for (owner, name), b in zip(poison.PATCHED, before))


def test_the_ctypes_scope_restores_the_binding(monkeypatch):
    """Against a stand-in for the binding module: this file needs no built library."""
    import sys
    import types
    stub = types.ModuleType("_gsr")
    stub.PYBIND = compiled = object()
    monkeypatch.setitem(sys.modules, "_gsr", stub)
    with poison.ctypes_binding():
        assert stub.PYBIND is None
    assert stub.PYBIND is compiled
    with pytest.raises(KeyError):
        with poison.ctypes_binding():
            assert stub.PYBIND is None
            raise KeyError("inside")
    assert stub.PYBIND is compiled


# ------------------------------------------------------------------ the package uses no allocation form the harness does not patch

# calls that hand out storage nobody has written.  `new_*` with an initial value (new_zeros, new_ones, new_full, new_tensor) are not among them.
UNINITIALISED = {"empty", "empty_like", "empty_strided", "empty_permuted", "empty_quantized", "new_empty", "new_empty_strided", "new", "resize_",
                 "resize_as_", "_empty_affine_quantized"}
TYPED_CONSTRUCTORS = {"Tensor", "FloatTensor", "DoubleTensor", "HalfTensor", "IntTensor", "LongTensor", "ShortTensor", "ByteTensor", "CharTensor",
                      "BoolTensor", "BFloat16Tensor"}


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    parts.append(node.id if isinstance(node, ast.Name) else "?")
    return ".".join(reversed(parts))


def scan_allocations(source, filename="<src>"):
    """[(line, form)] of the allocation calls in `source` that return uninitialised storage, `form` normalised to 'torch.empty',
    '.new_empty', ... ; a name imported from torch (`from torch import empty`) counts as 'import:<name>' — the patch would miss it."""
    found = []
    for node in ast.walk(ast.parse(source, filename)):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "torch":
            found += [(node.lineno, "import:" + a.name) for a in node.names if a.name in UNINITIALISED or a.name in TYPED_CONSTRUCTORS]
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        name = f.attr if isinstance(f, ast.Attribute) else f.id if isinstance(f, ast.Name) else None
        if name in TYPED_CONSTRUCTORS:
            # torch.Tensor([]) / torch.FloatTensor([1, 2]) build from data; torch.Tensor(3, 4) is uninitialised
            if not (len(node.args) == 1 and isinstance(node.args[0], (ast.List, ast.Tuple)) and not node.keywords):
                found.append((node.lineno, _dotted(f)))
        elif name in UNINITIALISED:
            if name == "new" and not isinstance(f, ast.Attribute):
                continue
            owner = _dotted(f.value) if isinstance(f, ast.Attribute) else ""
            found.append((node.lineno, ("torch." if owner == "torch" else "." if isinstance(f, ast.Attribute) else "") + name))
    return found


def test_the_scanner_sees_what_it_should():
    src = ("import torch\nfrom torch import empty\n"
           "a = torch.empty(3)\nb = torch.empty_like(a)\nc = a.new_empty((2,))\nd = torch.empty_strided((2,), (1,))\n"
           "e = a.new(4)\nf = torch.FloatTensor(3, 4)\ng = torch.Tensor([])\nh = a.new_zeros(3)\ni = torch.zeros(3)\n"
           "j = a.resize_(9)\nk = empty(3)\nl = torch.empty_permuted((2, 3), (1, 0))\nm = a.new_empty_strided((2,), (1,))\n"
           "n = x.y.new_empty(3)\n")
    got = scan_allocations(src)
    assert [f for _, f in sorted(got)] == ["import:empty", "torch.empty", "torch.empty_like", ".new_empty", "torch.empty_strided", ".new",
                                           "torch.FloatTensor", ".resize_", "empty", "torch.empty_permuted", ".new_empty_strided", ".new_empty"]


def test_the_package_allocates_only_through_the_patched_forms():
    files = sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    assert len(files) >= 20, files
    escaped, seen = [], 0
    for path in files:
        with open(path, encoding="utf-8") as fh:
            for line, form in scan_allocations(fh.read(), path):
                seen += 1
                if form not in poison.PATCHED_NAMES:
                    escaped.append("%s:%d %s" % (os.path.relpath(path, ROOT), line, form))
    assert seen >= 50          # the scan is live: the package has some eighty such calls
    assert not escaped, "allocation forms tests/poison.py does not patch:\n" + "\n".join(escaped)
    # and what the scan calls patched is what poisoned() patches
    assert poison.PATCHED_NAMES == {("torch." if owner is torch else ".") + name for owner, name in poison.PATCHED}
