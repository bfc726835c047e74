"""Every exported entry refuses every bad argument before any device work (include/gsr_hip.h: a bad argument returns GSR_E_INVALID,
"no kernel is launched").  The calls come from the table in tests/cabi_args.py — one row per entry, the status of every argument as the
header gives it — and run in ONE fresh child process that hides every GPU and asks the HIP runtime for the device count first: with a
device still visible nothing is called and the tests skip, because a missing check plus a fake pointer must never reach a real GPU.
Nothing here initialises a GPU."""
import sys

import pytest

import cabi_args
import cabi_child
import cabi_header
from cabi_args import NO_ARGUMENTS, ROWS, TABLE, WELL_FORMED


def _protos():
    """{entry: [argument names]} of include/gsr_hip.h."""
    return {name: cabi_header.arg_names(args) for _, name, args in cabi_header.protos(cabi_header.MAIN)}


def test_every_exported_entry_has_a_row(hip_lib_built):
    """A new entry cannot arrive untested: it needs a row, or a place among the entries that take neither a pointer nor a size."""
    import _gsr
    protos = _protos()
    assert sorted(protos) == sorted(_gsr.EXPORTED)
    assert not set(ROWS) & set(NO_ARGUMENTS)
    for entry in _gsr.EXPORTED:
        assert entry in ROWS or entry in NO_ARGUMENTS, f"{entry} is exported but tests/cabi_args.py has no row for it"
    for entry in NO_ARGUMENTS:
        assert not any("*" in a or a in ("P", "n", "width", "height", "H", "W", "C") for a in protos[entry]), entry
    assert sorted(set(ROWS) | set(NO_ARGUMENTS)) == sorted(protos), "a row for an entry the header does not declare"


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r.entry)
def test_row_lists_the_arguments_of_the_header_in_order(row):
    assert [a.name for a in row.args] == _protos()[row.entry]


@pytest.fixture(scope="module")
def outcomes(hip_lib_built):
    return cabi_child.run(__file__)


def test_workspace_check_puts_the_allocators_exception_first(hip_lib_built, monkeypatch):
    """_gsr.Workspace.check, without a device: an exception the allocation raised reaches the caller as that very object (the library's
    GSR_E_ALLOC hangs on it as its cause), and a GSR_E_ALLOC the callback did not cause is a GsrError."""
    import torch
    import _gsr
    ws = _gsr.Workspace("cpu")
    assert ws.check(7, "forward") == 7
    with pytest.raises(_gsr.GsrError, match="code -3"):
        ws.check(-3, "forward")
    assert ws.cb(None, _gsr.GSR_BUF_GEOM, 1024) and ws.error is None and ws.bufs[_gsr.GSR_BUF_GEOM].numel() == 1024
    injected = getattr(torch, "OutOfMemoryError", RuntimeError)("injected")

    class Failing:
        uint8 = torch.uint8

        @staticmethod
        def empty(*args, **kwargs):
            raise injected
    monkeypatch.setattr(_gsr, "torch", Failing)
    assert not ws.cb(None, _gsr.GSR_BUF_IMAGE, 1024)      # the library gets NULL ...
    monkeypatch.undo()
    with pytest.raises(type(injected)) as caught:          # ... answers GSR_E_ALLOC, and the caller gets the allocator's exception
        ws.check(-3, "forward")
    assert caught.value is injected and isinstance(caught.value.__cause__, _gsr.GsrError)
    assert ws.error is None


@pytest.mark.parametrize("entry, case", cabi_args.case_ids(), ids=lambda v: v)
def test_refusal(outcomes, entry, case):
    row = ROWS[entry]
    well_formed = case == WELL_FORMED or next(c for c in row.cases if c.id == case).ok
    if row.query:
        # a size query returns the size, and 0 for a size it has no answer for
        rc = cabi_child.reached(outcomes, entry, case)["rc"]
        assert (rc > 0) if well_formed else (rc == 0), (entry, case, rc)
        return
    # well-formed: whatever happens without a device (a HIP error, a refused allocation, success of a host-only entry), it is not a refusal:
    # the refusals come from the one changed argument
    got = cabi_child.check(outcomes, entry, case, "accepted" if well_formed else "refused", row.family)
    if not well_formed:
        assert got["allocs"] == 0, "the entry asked for workspace before refusing"


if __name__ == "__main__":
    sys.exit(cabi_child.serve(cabi_args.case_ids(), cabi_args.call))
