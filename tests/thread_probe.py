"""Tools for the host-thread tests (tests/test_gpu_threads.py, tests/test_threads_host.py).  Host-only: nothing here imports torch or
touches the GPU.

    run_threads(fns)         each callable on a daemon thread of its own; the return values in order; the first worker exception re-raised
                             in the caller with the worker's traceback.  A worker still alive after `timeout_s` is a hang: pytest.exit(),
                             naming the worker, so that nothing more is started on the GPU in that run.  (120 s is a guard, far above
                             anything a test here takes; it measures nothing.)
    Barrier / Event          threading's, with a timeout on every wait.  A barrier that breaks (a party failed or timed out) raises
                             BrokenRendezvous at every party at once: one worker failing never leaves the other one blocked.  run_threads
                             aborts the barriers it was given as soon as a worker fails.
    Span                     time.perf_counter() at entry and exit of a region; nested(inner, outer): `inner` lies wholly inside `outer`.

Not a conftest: tests import it."""
import threading
import time
import traceback

DEFAULT_TIMEOUT_S = 120.0
WAIT_TIMEOUT_S = 60.0


class BrokenRendezvous(RuntimeError):
    """A barrier was broken (another party failed, or did not arrive in time), or an event was not set in time."""


class WorkerError(RuntimeError):
    """A worker raised; the message carries the worker's own traceback."""


class Barrier:
    """threading.Barrier whose wait() has a timeout and raises BrokenRendezvous instead of threading.BrokenBarrierError."""

    def __init__(self, parties, timeout_s=WAIT_TIMEOUT_S, name="barrier"):
        self.name, self.timeout_s = name, float(timeout_s)
        self._barrier = threading.Barrier(parties)

    def wait(self, what=""):
        try:
            return self._barrier.wait(self.timeout_s)
        except threading.BrokenBarrierError:
            raise BrokenRendezvous("%s broken at %r: another party failed or did not arrive within %g s" % (self.name, what, self.timeout_s)) from None

    def abort(self):
        self._barrier.abort()

    @property
    def broken(self):
        return self._barrier.broken


class Event:
    """threading.Event whose wait() has a timeout and raises BrokenRendezvous when it runs out or the event was aborted."""

    def __init__(self, timeout_s=WAIT_TIMEOUT_S, name="event"):
        self.name, self.timeout_s = name, float(timeout_s)
        self._event, self._aborted = threading.Event(), False

    def set(self):
        self._event.set()

    def is_set(self):
        return self._event.is_set() and not self._aborted

    def wait(self, what=""):
        ok = self._event.wait(self.timeout_s)
        if self._aborted or not ok:
            raise BrokenRendezvous("%s %s at %r" % (self.name, "aborted: another party failed" if self._aborted else "not set within %g s" % self.timeout_s, what))

    def abort(self):
        self._aborted = True
        self._event.set()


class Span:
    """with Span() as s: ...   ->   s.t0, s.t1 (time.perf_counter()), s.seconds.  Span(t0, t1) makes one by hand."""

    def __init__(self, t0=None, t1=None):
        self.t0, self.t1 = t0, t1

    def __enter__(self):
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        self.t1 = time.perf_counter()
        return False

    @property
    def seconds(self):
        return self.t1 - self.t0

    def __repr__(self):
        return "Span(%r, %r)" % (self.t0, self.t1)


def nested(inner, outer):
    """True when both spans are closed and `inner` lies wholly inside `outer`: it began after `outer` began and ended before `outer`
    ended (strictly: two regions that share an end point did not demonstrably overlap)."""
    if None in (inner.t0, inner.t1, outer.t0, outer.t1) or inner.t1 < inner.t0 or outer.t1 < outer.t0:
        return False
    return outer.t0 < inner.t0 and inner.t1 < outer.t1


def run_threads(fns, timeout_s=DEFAULT_TIMEOUT_S, names=None, rendezvous=()):
    """Runs each of `fns` on its own daemon thread and returns their return values in order.  names: one per worker, for messages.
    rendezvous: the Barriers / Events the workers share; they are aborted as soon as one worker raises, so that the others fail at their
    next wait instead of sitting out its timeout.  The first exception (in time) is re-raised here as WorkerError, chained to the
    original, with the worker's traceback in the message; a BrokenRendezvous that merely followed another worker's failure is not the
    one reported.  A worker alive after `timeout_s` (all workers share the one deadline) counts as a hang: pytest.exit()."""
    import pytest
    fns = list(fns)
    names = list(names) if names is not None else ["worker %d" % i for i in range(len(fns))]
    assert len(names) == len(fns)
    results, errors, lock = [None] * len(fns), [], threading.Lock()

    def body(i):
        try:
            results[i] = fns[i]()
        except BaseException as ex:          # noqa: B902 (everything is reported to the caller)
            with lock:
                errors.append((i, ex, traceback.format_exc()))
            for r in rendezvous:
                r.abort()

    threads = [threading.Thread(target=body, args=(i,), name=names[i], daemon=True) for i in range(len(fns))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + float(timeout_s)
    for i, t in enumerate(threads):
        t.join(max(0.0, deadline - time.monotonic()))
        if t.is_alive():
            for r in rendezvous:
                r.abort()
            pytest.exit("thread_probe: %s is still running after %g s: a hang; nothing more is started in this run" % (names[i], timeout_s), returncode=3)
            raise RuntimeError("thread_probe: %s hung" % names[i])      # (only reached when pytest.exit is replaced by something that returns)
    if errors:
        first = [e for e in errors if not isinstance(e[1], BrokenRendezvous)] or errors
        i, ex, tb = first[0]
        raise WorkerError("%s raised %s: %s\n--- traceback of %s ---\n%s" % (names[i], type(ex).__name__, ex, names[i], tb)) from ex
    return results
