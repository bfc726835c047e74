"""tests/thread_probe.py on the CPU: a worker's exception reaches the caller with its traceback, a broken barrier raises at once instead of
being waited out, nested() tells overlap from order, and a worker that does not come back is reported as a hang by name.  The GPU tests
built on these tools (tests/test_gpu_threads.py) would pass vacuously, or block, were any of this wrong."""
import sys
import threading
import time

import pytest

import thread_probe as TP


def test_import_makes_no_gpu_call():
    assert "torch" not in vars(TP) and "thread_probe" in sys.modules


def test_return_values_come_back_in_order_from_threads_of_their_own():
    bar = TP.Barrier(2, timeout_s=30.0)

    def ident():
        mine = threading.get_ident()
        bar.wait("both alive")          # both workers are alive here: the system hands a finished thread's ident out again
        return mine
    idents = TP.run_threads([ident, ident, lambda: "c"], rendezvous=[bar])
    assert idents[2] == "c" and len({idents[0], idents[1], threading.get_ident()}) == 3
    assert TP.run_threads([]) == []


def test_a_worker_exception_is_raised_in_the_caller_with_the_workers_traceback():
    def a_function_with_a_telling_name():
        raise KeyError("the worker's own message")
    with pytest.raises(TP.WorkerError) as info:
        TP.run_threads([lambda: 1, a_function_with_a_telling_name], names=["first", "second"])
    text = str(info.value)
    assert "second raised KeyError" in text and "the worker's own message" in text
    assert "a_function_with_a_telling_name" in text and "Traceback" in text       # the worker's frames, not only the caller's
    assert isinstance(info.value.__cause__, KeyError)


def test_a_failing_worker_breaks_the_barrier_for_the_other_one_at_once():
    """Worker 0 raises before the barrier; worker 1 is already waiting there with a 30 s timeout.  It must get BrokenRendezvous at once,
    and the caller must be told about worker 0's error, not about the broken barrier that followed from it."""
    bar = TP.Barrier(2, timeout_s=30.0, name="step")
    waiting = TP.Event(timeout_s=30.0)
    seen = {}

    def fails():
        waiting.wait("worker 1 at the barrier")
        raise ValueError("first failure")

    def waits():
        waiting.set()
        try:
            bar.wait("after A.fwd")
        except TP.BrokenRendezvous as ex:
            seen["error"] = str(ex)
            raise
    t0 = time.perf_counter()
    with pytest.raises(TP.WorkerError) as info:
        TP.run_threads([fails, waits], rendezvous=[bar, waiting])
    assert time.perf_counter() - t0 < 10.0, "the barrier was waited out"
    assert "first failure" in str(info.value) and isinstance(info.value.__cause__, ValueError)
    assert "step broken" in seen["error"] and "after A.fwd" in seen["error"] and bar.broken


def test_a_barrier_nobody_else_reaches_raises_after_its_timeout_and_an_unset_event_too():
    bar = TP.Barrier(2, timeout_s=0.05)
    with pytest.raises(TP.BrokenRendezvous):
        bar.wait("alone")
    with pytest.raises(TP.BrokenRendezvous):          # a broken barrier stays broken: the next wait raises at once
        bar.wait("again")
    ev = TP.Event(timeout_s=0.05, name="go")
    with pytest.raises(TP.BrokenRendezvous, match="go not set"):
        ev.wait("never set")
    ev.abort()
    with pytest.raises(TP.BrokenRendezvous, match="aborted"):
        ev.wait("aborted")
    ok = TP.Event(timeout_s=0.05)
    ok.set()
    ok.wait("set")
    assert ok.is_set() and not ev.is_set()


def test_barriers_step_two_workers_in_the_order_written():
    bar = TP.Barrier(2, timeout_s=10.0)
    order = []

    def a():
        order.append("A1")
        bar.wait(1)
        bar.wait(2)
        order.append("A2")

    def b():
        bar.wait(1)
        order.append("B1")
        bar.wait(2)
    TP.run_threads([a, b], rendezvous=[bar])
    assert order == ["A1", "B1", "A2"]


def test_nested_on_hand_made_spans():
    outer = TP.Span(1.0, 5.0)
    assert TP.nested(TP.Span(2.0, 3.0), outer)
    assert TP.nested(TP.Span(1.0 + 1e-9, 5.0 - 1e-9), outer)
    assert not TP.nested(TP.Span(0.5, 3.0), outer)            # began earlier
    assert not TP.nested(TP.Span(2.0, 5.5), outer)            # ended later
    assert not TP.nested(TP.Span(5.0, 6.0), outer)            # after it: in order, no overlap
    assert not TP.nested(TP.Span(0.0, 1.0), outer)            # before it
    assert not TP.nested(outer, TP.Span(2.0, 3.0))            # the other way round
    assert not TP.nested(outer, outer)                        # shared end points show no overlap
    assert not TP.nested(TP.Span(1.0, 3.0), outer) and not TP.nested(TP.Span(3.0, 5.0), outer)
    assert not TP.nested(TP.Span(2.0, None), outer) and not TP.nested(TP.Span(2.0, 3.0), TP.Span(1.0, None))      # a span that never closed
    assert not TP.nested(TP.Span(3.0, 2.0), outer)            # not a span
    with TP.Span() as o:
        with TP.Span() as i:
            time.sleep(0.001)
        time.sleep(0.001)
    assert TP.nested(i, o) and not TP.nested(o, i) and 0 < i.seconds < o.seconds


def test_a_worker_that_does_not_come_back_is_reported_as_a_hang_by_name(monkeypatch):
    class Exited(Exception):
        pass

    def fake_exit(reason="", returncode=None):
        raise Exited(reason)
    monkeypatch.setattr(pytest, "exit", fake_exit)
    release = threading.Event()
    try:
        t0 = time.perf_counter()
        with pytest.raises(Exited) as info:
            TP.run_threads([lambda: 1, lambda: release.wait(20.0)], timeout_s=0.2, names=["quick", "sleeper"])
        assert time.perf_counter() - t0 < 5.0
        assert "sleeper" in str(info.value) and "quick" not in str(info.value) and "hang" in str(info.value)
    finally:
        release.set()                                         # (the daemon thread ends now instead of at its own timeout)
