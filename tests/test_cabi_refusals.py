"""Every exported entry refuses every bad argument before any device work (include/gsr_hip.h: a bad argument returns GSR_E_INVALID,
"no kernel is launched").  The calls come from the table in tests/cabi_args.py — one row per entry, the status of every argument as the
header gives it — and run in ONE fresh child process that hides every GPU and asks the HIP runtime for the device count first: with a
device still visible nothing is called and the tests skip, because a missing check plus a fake pointer must never reach a real GPU.
Nothing here initialises a GPU."""
import json
import os
import re
import subprocess
import sys

import pytest

import cabi_args
from cabi_args import GSR_E_INVALID, NO_ARGUMENTS, ROWS, TABLE, WELL_FORMED

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _protos():
    """{entry: [argument names]} of include/gsr_hip.h, parsed as tests/test_cabi.py does."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr_hip.h")).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"(?:int|size_t|const char\*)\s+(gsr_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        names = [re.sub(r".*[\s\*]", "", a.strip()) for a in args.split(",")]
        out[name] = [] if names == ["void"] else names
    return out


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
    """{(entry, case): outcome} of one run of the table in a child that sees no GPU; None when the child still saw one.  A case that takes
    the child down is recorded as such and the table resumes behind it in a new child (at most a few times)."""
    env = dict(os.environ, **cabi_args.HIDE_GPUS)
    done, extra = {}, []
    for _ in range(8):
        p = subprocess.run([sys.executable, os.path.join(HERE, "cabi_args.py")] + extra, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        begun = None
        for line in p.stdout.splitlines():
            if not line.startswith("{"):
                continue
            rec = json.loads(line)
            if "devices" in rec:
                if rec["devices"] != 0:
                    return None
            elif "begin" in rec:
                begun = tuple(rec["begin"])
            elif "done" in rec:
                done[tuple(rec["done"])] = rec
                begun = None
        if p.returncode == 0 and begun is None:
            break
        assert begun is not None, f"the child failed outside a call (exit {p.returncode}):\n{p.stderr[-3000:]}"
        done[begun] = {"crashed": p.returncode, "stderr": p.stderr[-500:]}
        extra = ["--after", begun[0], begun[1]]
    return done


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
    if outcomes is None:
        pytest.skip("a GPU is still visible to the child process although the visible-devices variables hide them: the table is not run")
    row = ROWS[entry]
    got = outcomes.get((entry, case))
    assert got is not None, "the child never reached this call"
    assert "crashed" not in got, f"the call took the process down (exit {got.get('crashed')}): {got.get('stderr')}"
    rc, msg, allocs = got["rc"], got["msg"], got["allocs"]
    well_formed = case == WELL_FORMED or next(c for c in row.cases if c.id == case).ok
    if row.query:
        # a size query returns the size, and 0 for a size it has no answer for
        assert (rc > 0) if well_formed else (rc == 0), (entry, case, rc)
        return
    if well_formed:
        # whatever happens without a device (a HIP error, a refused allocation, success of a host-only entry), it is not a refusal: the
        # refusals below come from the one changed argument
        assert rc != GSR_E_INVALID, (entry, rc, msg)
        return
    assert rc == GSR_E_INVALID, (entry, case, rc, msg)
    assert msg.startswith(row.family), (entry, case, msg)
    assert allocs == 0, "the entry asked for workspace before refusing"
