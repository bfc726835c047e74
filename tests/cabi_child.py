"""The child process in which the C-ABI tests call entries with fake pointers, and the parent's side of it.

A test file keeps its well-formed call and its case tables as data (`cases` lists them, `changes` looks one up), and ends in
    if __name__ == "__main__":
        sys.exit(cabi_child.serve(<[(entry, case)]>, <call(gsr, entry, case) -> rc>))
so that `python <that file>` is the child; its `outcomes` fixture is `cabi_child.run(__file__)` and its test_refusal calls `check`.  The
child hides every GPU and asks the HIP runtime for the device count first (tests/cabi_args.py's guard): with a device still visible
nothing is called and the tests skip, because a missing check plus a fake pointer must never reach a real GPU."""
import json
import os
import subprocess
import sys

import pytest

from cabi_args import GSR_E_INVALID, HIDE_GPUS, _visible_devices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STILL_VISIBLE = "a GPU is still visible to the child process although the visible-devices variables hide them: nothing is called"


def cases(entries, tables):
    """[(entry, case, expect)] of a file's case tables, ((expect, {entry: {case: changes}}), ...): entry by entry, and inside an entry
    table by table in the order given.  This is the order of the test ids and of the child's calls."""
    return [(entry, k, expect) for entry in entries for expect, table in tables for k in table.get(entry, {})]


def changes(tables, entry, case):
    """What `case` changes in the entry's well-formed call."""
    for _, table in tables:
        if case in table.get(entry, {}):
            return table[entry][case]
    raise KeyError(case)


def serve(cases, call, argv=None):
    """The child's loop over `cases`, [(entry, case)]: one JSON line before each call (so that a crash names its case) and one after it with
    the return code and gsr_last_error().  `call(gsr, entry, case)` makes the call and returns rc, or (rc, {further fields of the record}).
    `--after ENTRY CASE` resumes behind a case that took the process down."""
    argv = sys.argv[1:] if argv is None else argv
    os.environ.update(HIDE_GPUS)
    sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd"))
    import _gsr
    n = _visible_devices()
    print(json.dumps({"devices": n}), flush=True)
    if n != 0:
        return 0
    todo = [tuple(c) for c in cases]
    if "--after" in argv:
        i = argv.index("--after")
        todo = todo[todo.index((argv[i + 1], argv[i + 2])) + 1:]
    for entry, case in todo:
        print(json.dumps({"begin": [entry, case]}), flush=True)
        rc = call(_gsr, entry, case)
        rc, more = rc if isinstance(rc, tuple) else (rc, {})
        msg = _gsr.lib.gsr_last_error()
        print(json.dumps(dict({"done": [entry, case], "rc": int(rc), "msg": msg.decode(errors="replace") if msg else ""}, **more)), flush=True)
    return 0


def run(script):
    """{(entry, case): record} of one run of `script`'s cases in a child that sees no GPU; None when the child still saw one.  A case that
    takes the child down is recorded as {"crashed": exit code} and the table resumes behind it in a new child (at most 8 children)."""
    env = dict(os.environ, **HIDE_GPUS)
    done, extra = {}, []
    for _ in range(8):
        p = subprocess.run([sys.executable, os.path.abspath(script)] + extra, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
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


def reached(outcomes, entry, case):
    """The record of one call out of run()'s result: skips when that run still saw a GPU, fails when the call was not reached or took the
    child down."""
    if outcomes is None:
        pytest.skip(STILL_VISIBLE)
    got = outcomes.get((entry, case))
    assert got is not None, "the child never reached this call"
    assert "crashed" not in got, f"the call took the process down (exit {got.get('crashed')}): {got.get('stderr')}"
    return got


def check(outcomes, entry, case, expect, family=None):
    """The three expectations: "refused" (GSR_E_INVALID and a message that opens with the entry, or with its `family`), "accepted" (anything
    but a refusal: without a device the launch fails) and "noop" (returns 0).  Returns the record."""
    got = reached(outcomes, entry, case)
    if expect == "refused":
        assert got["rc"] == GSR_E_INVALID, (entry, case, got)
        assert got["msg"].startswith(family or entry), (entry, case, got["msg"])
    elif expect == "noop":
        assert got["rc"] == 0, (entry, case, got)
    else:
        assert expect == "accepted", expect
        assert got["rc"] != GSR_E_INVALID, (entry, case, got)
    return got
