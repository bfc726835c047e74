"""Two host threads on every stateful path: the contract of INTEGRATION.md, "Threads".

    every call is re-entrant per (host thread, device); the `num_rendered` read-back slot is `thread_local` per device
    (csrc/gsr_common.hip: readback_slot); the one side stream per device and its events sit behind a mutex (csrc/gsr_cubemap.hip); the
    asynchronous reflection tails of two threads share that stream and run in the order they were enqueued.

tests/test_gpu_streams.py drives the same state from ONE thread on several streams; here each stream has a host thread of its own.  The
views, the comparison and the serial-reference machinery are that module's, imported (not its autouse `negative_control` fixture, which
stays in its own namespace): view A = 4097 Gaussians at 200x136, view B = 257 at 96x64, cubemap L in {16, 128}.  This module picks its own
two streams with the same control (thread_streams below).

The reference is always the same work on the default stream, on the main thread, with nothing else in flight, computed once per key
(serial_ref); never a second multi-thread run.  Bars (as in the stream tests): forward outputs and integer state
bit-identical; gradients summed with float atomics 5e-5 of the tensor's maximum; cubemap and fail-value sinks after side_join 1e-5; a
non-finite value fails; an all-zero float reference is refused (test_gpu_streams.check).

Each worker enters its own `torch.cuda.stream(s)`: current stream and current device are thread-local in torch.  Every test ends with
torch.cuda.synchronize() and prints one `THREADS <family> <case>: ...` line.

The delay that holds thread A is not a fixed figure: max(50 ms, 20 x the serial duration of what thread B has to fit into it), that
duration measured in this process when B's serial reference is computed (after one untimed run, so that it is the cost of the work and
not of loading its kernels).  The factor leaves room for B's first call on a fresh thread (a new pinned word, a new event).

What is NOT promised, and not tested: the compiled binding (csrc/gsr_torch_binding.cpp) holds the GIL during a call, so two threads'
calls may serialise there (results are asserted, overlap is only reported); the gate of the key sort is a performance device that another
thread's backward may consume."""
import contextlib
import time

import numpy as np
import pytest
import torch

import stream_probe as SP
import test_gpu_streams as TS
import thread_probe as TP
from test_gpu_streams import KINDS, VIEWS, binding, check, drained, reads_poison

pytestmark = pytest.mark.gpu

ATOMIC, SINK = TS.ATOMIC, TS.SINK
CANDIDATES = 12
_streams = []
_ref, _seconds = {}, {}


# ------------------------------------------------------------------------------------------------------------ streams
@pytest.fixture(scope="module", autouse=True)
def thread_streams():
    """Two streams that run beside the default stream and beside each other, chosen by the control of the stream tests: an op issued
    without an event on one reads the poison of late inputs on the other, in both directions.  Two streams on one hardware queue
    serialise, and behind such a pair every test here would pass whatever the library did: without two such streams the module errors
    out."""
    default = torch.cuda.default_stream()
    tried = 0
    while len(_streams) < 2 and tried < CANDIDATES:
        c = torch.cuda.Stream()
        tried += 1
        with drained():
            for st in (c, default):
                with torch.cuda.stream(st):
                    torch.ones(4096, device="cuda") * 2
        if reads_poison(c, default) and reads_poison(default, c) and all(reads_poison(c, k) and reads_poison(k, c) for k in _streams):
            _streams.append(c)
        del c
    print("THREADS control: %d of %d candidate streams run beside the default stream and each other (unordered reads come back as poison, both ways)"
          % (len(_streams), tried))
    if len(_streams) < 2:
        raise RuntimeError("thread tests: only %d of %d candidate streams run beside the default stream and each other; two are needed" % (len(_streams), tried))
    yield


def streams():
    assert len(_streams) == 2, "the control has not chosen the streams"
    return tuple(_streams)


@contextlib.contextmanager
def synchronised():
    """Nothing in flight before; torch.cuda.synchronize() at the end, also behind a failure.  Not behind a hang (pytest.exit from
    run_threads): nothing more touches the GPU then."""
    torch.cuda.synchronize()
    try:
        yield
    except pytest.exit.Exception:
        raise
    except BaseException:
        torch.cuda.synchronize()
        raise
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the serial reference
def _L(kind, L):
    return 0 if kind in ("S", "G") else L


def serial_ref(kind, view, L, which="default"):
    """(results, seconds) of one whole view (forward, backward, results on the host) on the default stream, on the main thread, with
    nothing else in flight: computed once per key and never modified.  seconds: the duration of that computation, host fetch included,
    after one untimed run of the same work."""
    key = (kind, view, _L(kind, L), which)
    if key not in _ref:
        arrays, make = KINDS[kind](view, L)
        with drained():
            TS.host(TS.whole(make)(TS.on_device(arrays)))            # untimed: loads the kernels, warms the allocator
        with drained():
            t = TS.on_device(arrays)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _ref[key] = TS.host(TS.whole(make)(t))
            _seconds[key] = time.perf_counter() - t0
    return _ref[key], _seconds[key]


def delay_ms_for(seconds):
    return max(SP.DEFAULT_DELAY_MS, 20.0 * seconds * 1e3)


def worst(got, ref, keys):
    """(tensors of `exact` that differ in bits, worst deviation of `atomic`, of `sink`)"""
    bits = [k for k in keys.get("exact", ()) if not SP.same_bits(got[k], ref[k])]
    return bits, max([0.0] + [SP.deviation(got[k], ref[k]) for k in keys.get("atomic", ())]), max([0.0] + [SP.deviation(got[k], ref[k]) for k in keys.get("sink", ())])


def judge(family, case, pairs, measured=""):
    """pairs: [(name, got, ref, keys)].  Prints the THREADS line with the worst deviations of every pair, then asserts each with the
    stream tests' check()."""
    parts = []
    for name, got, ref, keys in pairs:
        bits, a, s = worst(got, ref, keys)
        parts.append("%s: %d of %d exact tensors differ%s, worst of the %g bar %.3g, of the %g bar %.3g"
                     % (name, len(bits), len(keys.get("exact", ())), (" %r" % (bits,)) if bits else "", ATOMIC, a, SINK, s))
    print("THREADS %s %s: %s%s" % (family, case, "; ".join(parts), ("; " + measured) if measured else ""))
    for name, got, ref, keys in pairs:
        check("threads " + family, "%s %s" % (case, name), got, ref, **keys)


def whole_view(stream, make, tensors):
    """Forward, backward, results (with side_join for the reflection views) and fetch of one view, all on `stream` alone."""
    with torch.cuda.stream(stream):
        v = make(tensors() if callable(tensors) else tensors)
        v.fwd()
        v.bwd()
        r = v.results()
    return SP.fetch(stream, r)


def ready(arrays):
    return lambda: TS.on_device(arrays)


# ============================================================================================== T1. the read-back slot per thread
@pytest.mark.parametrize("which", ["ctypes", "compiled"])
@pytest.mark.parametrize("variant", ["S", "G"])
def test_t1_readback_slot_per_thread(variant, which):
    """Thread A: late inputs on its stream, an event, then its forward, whose host sits in the library's `num_rendered` wait until the
    delay has run out.  Thread B, released by the event: the whole of the other view on the other stream.  Then A's backward.  The two
    views differ in num_rendered: a slot shared between the threads would hand A the count (and sequence number) of B.  With the ctypes
    binding, which releases the GIL, B's span must lie inside the span of A's forward call, or the test is vacuous; the compiled
    binding holds the GIL, so there the calls may serialise and the nesting is only reported."""
    with binding(which):
        ref_a, _ = serial_ref(variant, "A", 0, which)
        ref_b, sec_b = serial_ref(variant, "B", 0, which)
        assert int(ref_a["num_rendered"][0]) != int(ref_b["num_rendered"][0]) and int(ref_b["num_rendered"][0]) > 0
        ms = delay_ms_for(sec_b)
        (arr_a, make_a), (arr_b, make_b) = KINDS[variant]("A", 0), KINDS[variant]("B", 0)
        s_a, s_b = streams()
        go = TP.Event(name="A is about to call its forward")
        span = {}

        def a():
            with torch.cuda.stream(s_a):
                v = make_a(SP.late_inputs(s_a, arr_a, ms))
                with TP.Span() as span["A.fwd"]:
                    go.set()
                    v.fwd()
                v.bwd()
                r = v.results()
            return SP.fetch(s_a, r)

        def b():
            go.wait("B")
            with TP.Span() as span["B"]:
                return whole_view(s_b, make_b, ready(arr_b))
        with synchronised():
            got_a, got_b = TP.run_threads([a, b], names=["thread A", "thread B"], rendezvous=[go])
    is_nested = TP.nested(span["B"], span["A.fwd"])
    keys = TS.make_keys(variant)
    judge("T1", "%s %s" % (variant, which), [("A", got_a, ref_a, keys), ("B", got_b, ref_b, keys)],
          "delay %.1f ms, B serial %.2f ms, A.fwd took %.1f ms, B took %.1f ms, B nested in A.fwd: %s; num_rendered A %d B %d"
          % (ms, sec_b * 1e3, span["A.fwd"].seconds * 1e3, span["B"].seconds * 1e3, is_nested, int(got_a["num_rendered"][0]), int(got_b["num_rendered"][0])))
    if which == "ctypes":
        assert is_nested, ("vacuous: thread B did not run inside thread A's forward call", span)


# ============================================================================================== T2. short-lived threads
def test_t2_short_lived_threads():
    """View B (fused, asynchronous tail) three times, each in a fresh thread that is joined before the next starts, then once on the
    main thread; all four equal the serial reference.  Each thread exits WITHOUT joining the side stream, so its scratch stays in
    `_gsr._side_held` behind a dead thread (and its `thread_local` read-back slot behind it); the results of run k are collected, with
    side_join, by the thread of run k + 1 and those of the third by the main thread."""
    import _gsr
    kind, L = "fused_async", 16
    ref, sec = serial_ref(kind, "B", L)
    arrays, make = KINDS[kind]("B", L)
    s_b = streams()[1]
    dev = torch.cuda.current_device()
    got, pending, left = [], [], []

    def run():
        out = None
        with torch.cuda.stream(s_b):
            if pending:
                out = SP.fetch(s_b, pending.pop().results())
            v = make(TS.on_device(arrays))
            v.fwd()
            v.bwd()
            pending.append(v)
        return out
    with synchronised():
        first = TP.run_threads([run], names=["short-lived thread 1"])[0]
        left.append(len(_gsr._side_held.get(dev, [])))
        got.append(TP.run_threads([run], names=["short-lived thread 2"])[0])
        left.append(len(_gsr._side_held.get(dev, [])))
        got.append(TP.run_threads([run], names=["short-lived thread 3"])[0])
        left.append(len(_gsr._side_held.get(dev, [])))
        with torch.cuda.stream(s_b):
            got.append(SP.fetch(s_b, pending.pop().results()))
        got.append(whole_view(s_b, make, ready(arrays)))
    assert first is None and len(got) == 4 and all(n > 0 for n in left), ("no scratch was left behind by an exited thread", left)
    keys = TS.make_keys(kind)
    judge("T2", "%s view B" % kind, [("thread %d" % (i + 1) if i < 3 else "main thread", g, ref, keys) for i, g in enumerate(got)],
          "B serial %.2f ms; tensors held for the side stream when threads 1-3 had exited: %r" % (sec * 1e3, left))


# ============================================================================================== T3. the shared side stream
ASYNC_KINDS = ["fused_async", "two_node_async"]


def _stepped(order, fns):
    """order: e.g. ["A.fwd", "B.fwd", "A.bwd", "B.bwd"]; fns: {"A": {"fwd": f, "bwd": f}, ...}.  Returns one worker body per thread that
    does its own steps in turn, with a barrier after every step."""
    bar = TP.Barrier(len(fns), name="step barrier")

    def body(me):
        def walk():
            for step in order:
                who, what = step.split(".")
                if who == me:
                    fns[me][what]()
                bar.wait(step)
        return walk
    return bar, {me: body(me) for me in fns}


@pytest.mark.parametrize("L", TS.SIZES)
@pytest.mark.parametrize("order", ["ABAB", "ABBA"])
@pytest.mark.parametrize("kind", ASYNC_KINDS)
def test_t3_phase_stepped(kind, order, L):
    """Two threads, each with its own stream, leaves and FlatGrads, stepped by barriers through A.fwd, B.fwd and the backwards in either
    order; then each joins the side stream on its own stream and fetches on that stream alone."""
    refs = {v: serial_ref(kind, v, L)[0] for v in "AB"}
    steps = ["A.fwd", "B.fwd"] + (["A.bwd", "B.bwd"] if order == "ABAB" else ["B.bwd", "A.bwd"])
    st = dict(zip("AB", streams()))
    views = {}

    def under(v, what):
        def fn():
            with torch.cuda.stream(st[v]):
                if what == "fwd":
                    arrays, make = KINDS[kind](v, L)
                    views[v] = make(TS.on_device(arrays))
                getattr(views[v], what)()
        return fn
    bar, walk = _stepped(steps, {v: {"fwd": under(v, "fwd"), "bwd": under(v, "bwd")} for v in "AB"})

    def worker(v):
        def fn():
            walk[v]()
            with torch.cuda.stream(st[v]):
                r = views[v].results()
            return SP.fetch(st[v], r)
        return fn
    with synchronised():
        got_a, got_b = TP.run_threads([worker("A"), worker("B")], names=["thread A", "thread B"], rendezvous=[bar])
    keys = TS.make_keys(kind)
    judge("T3 stepped", "%s %s L=%d" % (kind, order, L), [("A", got_a, refs["A"], keys), ("B", got_b, refs["B"], keys)], "steps " + " ".join(steps))


@pytest.mark.parametrize("which", ["ctypes", "compiled"])
@pytest.mark.parametrize("L", TS.SIZES)
@pytest.mark.parametrize("kind", ASYNC_KINDS)
def test_t3_nested(kind, L, which):
    """As T1: A's forward is held by late inputs (the camera ready, see test_gpu_streams.ready_camera) while B runs forward, backward,
    side_join and fetch inside it; then A's backward, side_join and fetch.  Nesting is asserted under ctypes."""
    with binding(which):
        ref_a, _ = serial_ref(kind, "A", L, which)
        ref_b, sec_b = serial_ref(kind, "B", L, which)
        ms = delay_ms_for(sec_b)
        (arr_a, make_a), (arr_b, make_b) = KINDS[kind]("A", L), KINDS[kind]("B", L)
        fixed = TS.ready_camera(arr_a, TS.refl_arrays("A", L)[1])
        late_a = {k: v for k, v in arr_a.items() if k not in fixed}
        s_a, s_b = streams()
        go = TP.Event(name="A is about to call its forward")
        span = {}

        def a():
            with torch.cuda.stream(s_a):
                v = make_a(dict(SP.late_inputs(s_a, late_a, ms), **fixed))
                with TP.Span() as span["A.fwd"]:
                    go.set()
                    v.fwd()
                v.bwd()
                r = v.results()
            return SP.fetch(s_a, r)

        def b():
            go.wait("B")
            with TP.Span() as span["B"]:
                return whole_view(s_b, make_b, ready(arr_b))
        with synchronised():
            got_a, got_b = TP.run_threads([a, b], names=["thread A", "thread B"], rendezvous=[go])
    is_nested = TP.nested(span["B"], span["A.fwd"])
    keys = TS.make_keys(kind)
    judge("T3 nested", "%s L=%d %s" % (kind, L, which), [("A", got_a, ref_a, keys), ("B", got_b, ref_b, keys)],
          "delay %.1f ms, B serial %.2f ms, A.fwd took %.1f ms, B took %.1f ms, B nested in A.fwd: %s"
          % (ms, sec_b * 1e3, span["A.fwd"].seconds * 1e3, span["B"].seconds * 1e3, is_nested))
    if which == "ctypes":
        assert is_nested, ("vacuous: thread B did not run inside thread A's forward call", span)


@pytest.mark.parametrize("L", TS.SIZES)
@pytest.mark.parametrize("kind", ASYNC_KINDS)
def test_t3_tail_behind_a_held_tail(kind, L):
    """A.fwd, then on A's stream a delay in front of the upstream gradients of A's backward (poison until it has run out), then A.bwd,
    enqueued without a host wait: A's tail sits on the side stream behind A's fork event.  A barrier; B runs forward, backward with its
    asynchronous tail, side_join and fetch: its sinks must be complete and correct although A's tail is queued in front of them.  Then
    A's sinks: anything of A that ran early has read the poison.  Vacuous, and failed as such, if A's stream had already run dry when B
    began."""
    ref_a, _ = serial_ref(kind, "A", L)
    ref_b, sec_b = serial_ref(kind, "B", L)
    ms = delay_ms_for(sec_b)
    (arr_a, make_a), (arr_b, make_b) = KINDS[kind]("A", L), KINDS[kind]("B", L)
    s_a, s_b = streams()
    bar = TP.Barrier(2, name="step barrier")
    seen = {}

    def a():
        with torch.cuda.stream(s_a):
            t = TS.on_device(arr_a)
            v = make_a(t)
            v.fwd()
            up = SP.late_inputs(s_a, {k: arr_a[k] for k in ("up_final", "up_allmap")}, ms)
            t.update(up)
            v.bwd()
            seen["end of A.bwd"] = torch.cuda.Event()
            seen["end of A.bwd"].record(s_a)
        bar.wait("A.bwd is enqueued")
        bar.wait("B is done")
        with torch.cuda.stream(s_a):
            r = v.results()
        return SP.fetch(s_a, r)

    def b():
        bar.wait("A.bwd is enqueued")
        seen["A held when B began"] = not seen["end of A.bwd"].query()
        with TP.Span() as seen["B"]:
            got = whole_view(s_b, make_b, ready(arr_b))
        bar.wait("B is done")
        return got
    with synchronised():
        got_a, got_b = TP.run_threads([a, b], names=["thread A", "thread B"], rendezvous=[bar])
    keys = TS.make_keys(kind)
    judge("T3 held tail", "%s L=%d" % (kind, L), [("B", got_b, ref_b, keys), ("A", got_a, ref_a, keys)],
          "delay %.1f ms, B serial %.2f ms, B took %.1f ms, A's backward still held when B began: %s" % (ms, sec_b * 1e3, seen["B"].seconds * 1e3, seen["A held when B began"]))
    assert seen["A held when B began"], "vacuous: A's stream had run dry before B began"


# ============================================================================================== T5. stage timers
def test_t5_stage_timers_count_both_threads():
    """With profiling on, the per-stage launch counts of both views run on two threads at once equal the sum of the counts of view A
    alone and of view B alone; every stage's time is finite and not negative.  (The records and their free list sit behind a mutex,
    csrc/gsr_common.hip.)"""
    import _gsr
    kind, L = "fused_async", 16
    refs = {v: serial_ref(kind, v, L)[0] for v in "AB"}
    st = dict(zip("AB", streams()))
    with synchronised():
        _gsr.profile_enable(True)
        try:
            alone = {}
            for v in "AB":
                arrays, make = KINDS[kind](v, L)
                _gsr.profile_collect()
                whole_view(torch.cuda.default_stream(), make, ready(arrays))
                torch.cuda.synchronize()
                alone[v] = _gsr.profile_collect()
            got = TP.run_threads([lambda v=v: whole_view(st[v], KINDS[kind](v, L)[1], ready(KINDS[kind](v, L)[0])) for v in "AB"], names=["thread A", "thread B"])
            torch.cuda.synchronize()
            both = _gsr.profile_collect()
        finally:
            _gsr.profile_enable(False)
    want = {s: alone["A"][s][1] + alone["B"][s][1] for s in _gsr.STAGES}
    have = {s: both[s][1] for s in _gsr.STAGES}
    keys = TS.make_keys(kind)
    judge("T5", kind, [("A", got[0], refs["A"], keys), ("B", got[1], refs["B"], keys)],
          "launches per stage, two threads / A alone + B alone: " + ", ".join("%s %d/%d" % (s, have[s], want[s]) for s in _gsr.STAGES if want[s] or have[s]))
    assert sum(want.values()) > 0 and all(alone[v]["render_fwd"][1] > 0 and alone[v]["refl_bwd_tail"][1] > 0 for v in "AB"), alone
    assert have == want
    for table in (alone["A"], alone["B"], both):
        assert all(np.isfinite(ms) and ms >= 0 for ms, _ in table.values()), table


# ============================================================================================== T6. viewer beside trainer
STEPS = FRAMES = 6
ITEMS = ["RGB", "Alpha", "Normal", "Base Color", "Refl. Strength", "Curvature"]          # frame i shows mode i


LR_SCALE = 1e-3


def _trainer(stream):
    """6 training steps through the drop-in API on `stream`, view A's size, L = 16: render() with the gradient sinks and the asynchronous
    reflection tail, l1_loss, ssim, backward(), one GaussianTrainState step.  Returns the per-step losses, each step's gradients, the
    parameters after step 1 and after step 6, on the host.

    The learning rates are the defaults times LR_SCALE.  With the defaults themselves six steps from this start are not one trajectory
    but two: Adam divides by sqrt(v) + 1e-15, so the 1e-7 of the float atomics' order becomes 1e-6 of the parameters by step 4, and at
    step 5 that decides on which side of a discontinuity of the renderer's gradient the step lands.  Measured on an MI355X, three
    sessions, SERIAL runs on the default stream included: runs agree to 1e-6 .. 6e-6 of every tensor up to step 4 and then either stay
    there (9e-5 at the end) or part: step 5's gradients differ by 0.095 (means3D), 0.1 (rotations), 0.017 (opacities) of their maxima,
    the end states by 0.0123 (opacities), 0.0087 (cubemap), 0.0078 (scales), the losses by 3e-6; always the same two branches, a serial
    run on either (serial / serial / beside the viewer: first, first, second in one session; first, second, second in another; all on
    one in a third).  One measured serial-to-serial spread cannot stand for that.  A thousandth of the rates keeps the amplified noise
    near 1e-9, three orders below what took the two branches apart.  The end state then moves little against the 5e-5 bar, so each
    step's gradients, which a race would corrupt first, are compared as well, at the same margin."""
    from gaussian_renderer import render
    from gsr_train import DEFAULT_LRS, GaussianTrainState
    from utils.loss_utils import l1_loss, ssim
    arrays, cam = TS.refl_arrays("A", 16)
    _, W, H, seed, _, _ = VIEWS["A"]
    with torch.cuda.stream(stream):
        t = TS.on_device(arrays)
        gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(seed)).cuda()
        rates = {k: v * LR_SCALE for k, v in DEFAULT_LRS.items() if k.endswith(("_lr", "_lr_init", "_lr_final"))}
        state = GaussianTrainState({k: t[k] for k in TS.PARAMS}, "cuda", lrs=rates)
        _, View = TS._model_and_view(t, cam)

        class Env:
            params = {"Cubemap_texture": state.p["cubemap"], "Cubemap_failv": state.p["fail"]}

        class PC:
            get_xyz, get_opacity, get_scaling, get_rotation, get_features, get_refl = (state.p["means3D"], state.p["opacities"], state.p["scales"],
                                                                                       state.p["rotations"], state.p["shs"], state.p["refl_strengths"])
            active_sh_degree, get_envmap = 3, Env

        class Pipe:
            depth_ratio, compute_cov3D_python = 0.0, False
            gsr_grad_sink, gsr_reflection_grad_sink = state.grads.sink(), state.grads.sink(names=("cubemap", "fail"))
            gsr_accumulate, gsr_async_reflection_tail = False, True
        out, losses = {}, []
        for step in range(STEPS):
            state.grads.zero_()
            pkg = render(View, PC, Pipe, t["bg"])
            l1, ss = l1_loss(pkg["render"], gt), ssim(pkg["render"], gt)
            loss = 0.8 * l1 + 0.2 * (1.0 - ss)
            loss.backward()
            state.optimizer.step()                  # (joins the side stream: the gradients are complete behind it, and it does not change them)
            losses.append(loss.detach())
            out.update({"g%d_%s" % (step, k): state.grads.view(k).clone() for k in TS.PARAMS})
            if step == 0:
                out.update({"one_" + k: state.p[k].detach().clone() for k in TS.PARAMS})
        out["loss"] = torch.stack(losses)
        out.update({"six_" + k: state.p[k].detach() for k in TS.PARAMS})
    return SP.fetch(stream, out)


def _viewer(stream):
    """6 frames on `stream`: render_fast() under no_grad and present_bytes, view B's camera, a frozen model with tensors of its own."""
    from gaussian_renderer import render_fast
    from test_gpu_dropin import _Pipe
    from utils import image_utils as IU
    arrays, cam = TS.refl_arrays("B", 16)
    with torch.cuda.stream(stream):
        t = TS.on_device(arrays)
        PC, View = TS._model_and_view(t, cam)
        frames = {}
        with torch.no_grad():
            for i in range(FRAMES):
                pkg = render_fast(View, PC, _Pipe, t["bg"])
                frames["frame%d" % i] = IU.present_bytes(pkg["render"], pkg, ITEMS, i)
    return SP.fetch(stream, frames)


def test_t6_viewer_beside_trainer():
    """Free-running on purpose: a trainer thread and a viewer thread through the drop-in API, exercising `_cached_block`, the
    (device, stream) scratch of image_utils, `_side_held` and `_last_sums` together.  (A viewer that reads parameters while Adam writes
    them is the caller's race: the viewer's model is a second, frozen one.)  Every frame is bit-identical to the serial frame.  Step 1's
    loss is bit-identical; the parameters after one step meet the gradient bar.  For the later losses and the end state after six steps
    the margin is not picked in advance: the serial run is measured once against a second serial run, and that spread plus the atomic
    bar is the margin, per tensor.  Each step's gradients are held to the same margin, and those of step 1, which start from the same
    bits, to the bars themselves (see _trainer for why the learning rates are a thousandth of the defaults)."""
    default = torch.cuda.default_stream()
    if "t6" not in _ref:
        with drained():
            _ref["t6"] = (_trainer(default), _viewer(default))
        with drained():
            _ref["t6 again"] = _trainer(default)
    (ref_t, ref_v), again = _ref["t6"], _ref["t6 again"]
    s_a, s_b = streams()
    with synchronised():
        got_t, got_v = TP.run_threads([lambda: _trainer(s_a), lambda: _viewer(s_b)], names=["trainer thread", "viewer thread"])
    frames = tuple("frame%d" % i for i in range(FRAMES))
    assert all(ref_v[f].dtype == np.uint8 and ref_v[f].max() > ref_v[f].min() for f in frames), "a serial frame shows nothing"
    assert not any(SP.same_bits(ref_v[frames[i]], ref_v[frames[j]]) for i in range(FRAMES) for j in range(i)), "two modes gave one frame"
    one, six = tuple("one_" + k for k in TS.PARAMS), tuple("six_" + k for k in TS.PARAMS)
    assert np.isfinite(ref_t["loss"]).all() and ref_t["loss"][-1] != ref_t["loss"][0], ref_t["loss"]
    grads = tuple("g%d_%s" % (i, k) for i in range(STEPS) for k in TS.PARAMS)
    assert all(np.abs(ref_t[k]).max() > 0 for k in grads if not k.endswith("_fail")), "a serial gradient is all zero"
    assert all(np.abs(ref_t["six_" + k] - ref_t["one_" + k]).max() > 0 for k in TS.PARAMS[:7]), "steps 2 to 6 moved nothing"
    spread = {k: SP.deviation(again[k], ref_t[k]) for k in six + grads}
    spread["loss"] = SP.deviation(again["loss"][1:], ref_t["loss"][1:])
    dev6 = {k: SP.deviation(got_t[k], ref_t[k]) for k in six + grads}
    dev6["loss"] = SP.deviation(got_t["loss"][1:], ref_t["loss"][1:])
    dev1 = {k: SP.deviation(got_t[k], ref_t[k]) for k in one}
    bad_frames = [f for f in frames if not SP.same_bits(got_v[f], ref_v[f])]
    print("THREADS T6 free-running: %d of %d frames differ; loss of step 1 bit-identical: %s; after one step worst of the %g bar %.3g; six steps, "
          "deviation / margin (serial-to-serial spread + %g): %s"
          % (len(bad_frames), FRAMES, SP.same_bits(got_t["loss"][:1], ref_t["loss"][:1]), ATOMIC, max(dev1.values()), ATOMIC,
             ", ".join("%s %.3g/%.3g" % (k.replace("six_", ""), dev6[k], spread[k] + ATOMIC) for k in ("loss",) + six))
          + "; gradients of the six steps, worst deviation %.3g, worst serial-to-serial spread %.3g" % (max(dev6[k] for k in grads), max(spread[k] for k in grads)))
    check("threads T6", "viewer frames", got_v, ref_v, exact=frames)
    assert SP.same_bits(got_t["loss"][:1], ref_t["loss"][:1]), (got_t["loss"], ref_t["loss"])
    check("threads T6", "parameters after one step", got_t, ref_t, atomic=one, may_be_zero=())
    check("threads T6", "gradients of step 1", got_t, ref_t, atomic=tuple("g0_" + k for k in TS.PARAMS[:6]), sink=("g0_cubemap", "g0_fail"),
          may_be_zero=("g0_fail",))
    late = [(k, dev6[k], spread[k] + ATOMIC) for k in dev6 if not dev6[k] <= spread[k] + ATOMIC]
    assert not late, late


def test_t6_l1_and_ssim_with_another_threads_l1_in_between():
    """Stepped by barriers: A calls l1_loss(imgA, gtA); B calls l1_loss(imgB, gtB), which replaces `loss_utils._last_sums`; A calls
    ssim(imgA, gtA) and backward().  A's values and gradient equal the serial ones, bit for bit (the same kernels on the same inputs:
    A's ssim() merely runs the fused forward again instead of sharing A's first one)."""
    import loss_bounds as LB
    from utils.loss_utils import clear_cache, l1_loss, ssim
    pairs = {"A": LB.loss_pair("uniform", (3,) + VIEWS["A"][2:0:-1], 72), "B": LB.loss_pair("uniform", (3,) + VIEWS["B"][2:0:-1], 73)}
    st = dict(zip("AB", streams()))

    def serial(t):
        clear_cache()
        x = t["x"].clone().requires_grad_(True)
        l1, ss = l1_loss(x, t["y"]), ssim(x, t["y"])
        ss.backward()
        clear_cache()
        return dict(l1=l1, ssim=ss, grad=x.grad)
    ref = TS.serial(("threads", "t6 l1 ssim"), dict(x=pairs["A"][0], y=pairs["A"][1]), serial)
    bar = TP.Barrier(2, name="step barrier")
    seen = {}

    def a():
        with torch.cuda.stream(st["A"]):
            t = TS.on_device(dict(x=pairs["A"][0], y=pairs["A"][1]))
            x = t["x"].clone().requires_grad_(True)
            l1 = l1_loss(x, t["y"])
            bar.wait("A.l1")
            bar.wait("B.l1")
            import utils.loss_utils as LU
            seen["replaced"] = LU._last_sums is not None and LU._last_sums[0]() is not x
            ss = ssim(x, t["y"])
            ss.backward()
            out = dict(l1=l1, ssim=ss, grad=x.grad)
        return SP.fetch(st["A"], out)

    def b():
        with torch.cuda.stream(st["B"]):
            t = TS.on_device(dict(x=pairs["B"][0], y=pairs["B"][1]))
            bar.wait("A.l1")
            l1 = l1_loss(t["x"], t["y"])
            bar.wait("B.l1")
        return SP.fetch(st["B"], dict(l1=l1))
    clear_cache()
    try:
        with synchronised():
            got_a, got_b = TP.run_threads([a, b], names=["thread A", "thread B"], rendezvous=[bar])
    finally:
        clear_cache()
    judge("T6 stepped", "l1 A, l1 B, ssim A", [("A", got_a, ref, dict(exact=("l1", "ssim", "grad")))], "B's l1_loss replaced A's shared sums: %s" % seen["replaced"])
    assert seen["replaced"], "vacuous: thread B's l1_loss did not replace the shared sums"
    assert np.isfinite(got_b["l1"]).all() and got_b["l1"] > 0
