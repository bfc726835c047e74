"""The C-ABI library must load on a machine without a GPU, and every header under include/ must agree with the library and with the one
table of the ctypes binding (_gsr.ABI): the same entries, exported, with the argument and return types of the prototypes, and descriptor
structs with the header's fields.  Every include/gsr_hip*.h is tested the same way (tests/cabi_header.py finds and parses them).  No
compute entry point is called here (CPU-only suite)."""
import ctypes
import os
import re

import pytest

import cabi_header as hdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("header", hdr.headers())
def test_library_loads_and_exports_every_declared_symbol(hip_lib_built, header):
    import _gsr
    raw = ctypes.CDLL(_gsr.LIB_PATH)
    names = [n for _, n, _ in hdr.protos(header)]
    assert names, header
    for n in names:
        assert hasattr(raw, n), f"{n} declared in {header} but not exported by libgsr_hip.so"
    assert sorted(names) == sorted(_gsr.ENTRIES_BY_HEADER[header]), header
    if header == hdr.MAIN:
        assert len(names) >= 14 and _gsr.EXPORTED == _gsr.ENTRIES_BY_HEADER[header]


@pytest.mark.parametrize("header", hdr.headers())
def test_ctypes_signatures_match_header(hip_lib_built, header):
    import _gsr
    for ret, name, args in hdr.protos(header):
        if name not in _gsr.ENTRIES_BY_HEADER[header]:
            continue                 # (an entry without a row: the test above names it)
        fn = getattr(_gsr.lib, name)
        assert [hdr.ctype(a) for a in args] == list(fn.argtypes or []), (header, name)
        assert fn.restype is hdr.restype(ret), (header, name)


@pytest.mark.parametrize("header", hdr.headers())
def test_descriptor_structs_match_header(hip_lib_built, header):
    """Every struct a header defines: the same fields in the same order, with the same types, as its class in the binding."""
    import _gsr
    for c_name in hdr.structs(header):
        assert c_name in hdr.STRUCTS, f"{header} defines {c_name}, which tests/cabi_header.py maps to no class of _gsr"
        assert hdr.struct_fields(header, c_name) == list(getattr(_gsr, hdr.STRUCTS[c_name])._fields_), (header, c_name)


@pytest.mark.parametrize("header", [h for h in hdr.headers() if h != hdr.MAIN])
def test_later_header_includes_the_main_header_and_leaves_the_version_to_it(header):
    assert re.search(r'#include "gsr_hip\.h"', hdr.text(header))
    assert "GSR_ABI_VERSION" not in hdr.text(header)             # the version is the main header's, and stays


def test_every_entry_is_declared_in_one_header_and_sits_in_one_group(hip_lib_built):
    import _gsr
    declared = [(n, h) for h in hdr.headers() for _, n, _ in hdr.protos(h)]
    bound = [(row[0], header) for header, _, _, rows in _gsr.ABI for row in rows]
    for where, pairs in (("declared", declared), ("in _gsr.ABI", bound)):
        names = [n for n, _ in pairs]
        twice = sorted({n for n in names if names.count(n) > 1})
        assert not twice, f"{where} more than once: {[(n, [h for m, h in pairs if m == n]) for n in twice]}"
    assert sorted(_gsr.ENTRIES_BY_HEADER) == hdr.headers()        # (header by header, the parametrised test above compares the names)
    for n, h in declared:                   # (nor does another header mention it outside a comment)
        for other in hdr.headers():
            assert other == h or not re.search(r"\b%s\b" % n, hdr.source(other)), (n, other)
    for _, source, _, rows in _gsr.ABI:     # the file require_entry names is where the entry is defined
        text = open(os.path.join(ROOT, "gaussian-splatting-reflection_amd", source)).read()
        for row in rows:
            assert re.search(r'extern "C" [\w\s\*]*\b%s\s*\(' % row[0], text), (row[0], source)


def test_abi_version_is_102_in_header_binding_and_library(hip_lib_built):
    """The library and the binding agree on the ABI version the header states (a binding written against another header refuses to load)."""
    import _gsr
    assert _gsr.lib.gsr_version() == _gsr.GSR_ABI_VERSION == int(re.search(r"#define GSR_ABI_VERSION (\d+)", hdr.text(hdr.MAIN)).group(1)) == 102


def test_activation_kinds_match_header(hip_lib_built):
    import _gsr
    src = hdr.source("gsr_hip_train.h")
    for k, v in (("NONE", _gsr.GSR_ACT_NONE), ("SIGMOID", _gsr.GSR_ACT_SIGMOID), ("EXP", _gsr.GSR_ACT_EXP), ("NORMALIZE4", _gsr.GSR_ACT_NORMALIZE4),
                 ("FROZEN", _gsr.GSR_ACT_FROZEN)):
        assert int(re.search(r"#define GSR_ACT_%s (\w+)" % k, src).group(1), 0) == v


def test_require_entry_names_the_entry_its_source_file_and_the_rebuild(hip_lib_built):
    import _gsr
    _gsr.require_entry(_gsr.lib, "gsr_envmap_sharpen")
    with pytest.raises(ImportError, match=r"does not export gsr_envmap_sharpen \(csrc/gsr_envmap\.hip\).*rebuild with .*build\.py --force.*no torch fallback"):
        _gsr.require_entry(object(), "gsr_envmap_sharpen")


def test_host_only_entry_points(hip_lib_built):
    """Calls that never touch the device: option switches, error strings, argument validation."""
    import _gsr
    assert _gsr.lib.gsr_set_option(b"cull", 1) == 0
    assert _gsr.lib.gsr_set_option(b"no-such-option", 1) == -1
    assert b"no-such-option" in _gsr.lib.gsr_last_error()
    with pytest.raises(_gsr.GsrError):
        _gsr.set_option("bogus", 1)
    # profiling bookkeeping works without a device as long as nothing was recorded
    _gsr.profile_enable(False)
    assert all(v == (0.0, 0) for v in _gsr.profile_collect().values())


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    """There is no CPU fallback: importing the binding without the .so raises ImportError."""
    import importlib.util
    src = os.path.join(ROOT, "gaussian-splatting-reflection_amd", "_gsr.py")
    dst = tmp_path / "_gsr_copy.py"
    dst.write_text(open(src).read())
    spec = importlib.util.spec_from_file_location("_gsr_copy", str(dst))
    mod = importlib.util.module_from_spec(spec)
    with pytest.raises(ImportError, match="no CPU fallback|not found"):
        spec.loader.exec_module(mod)
