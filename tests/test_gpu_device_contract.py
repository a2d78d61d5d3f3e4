"""The device entry points as the solver calls them: asynchronous on torch's
current stream, out of a workspace cached per stream, captured into graphs and
replayed, and behind them the host layer's persistent state. The arithmetic is
held to its bounds elsewhere (test_gpu_pair_accuracy.py); what is checked here
is that a launch goes where and when its stream says, so nearly everything is
bit-equality with the same launch done the plain way (default stream, one call
at a time), and `judge` with the longdouble references of pair_reference.py
where a result is new.

Shapes (tests/pair_cases.py), the smallest that reach each mechanism:
  SMALL    131 x 513: two chunks and a tail, 2 targets a thread, in 1 and 3
           forced slices (3: the partials and the reduction);
  LONG     1300 x 1100, the launch that outgrows SMALL's workspace block;
  NEAR     coincident and regularized pairs;
  PLANNED  400 x 4099, the one shape the planner itself may split (at most
           ceil(4099 / 2048) = 3 slices; bounded with 3, and R.bound grows
           with the slice count).
A second value set of a shape is another seed at the same counts.

No test here passes a mismatched length, a bad `out` or a negative count to a
real launch: the argument tests run against a library that raises when it is
touched. Every test sets the workspace, slice and fast-path switches it wants
and puts them back to their defaults, workspace persistent / planner's slices
/ fast path auto (other tests leave the workspace switch forced on or off for
the rest of the process, so none may assume its state)."""

import threading
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest

import pair_cases as PC
import pair_reference as R
from test_gpu_pair_accuracy import EVALUATE, judge
from test_gpu_pair_slices import sliced

pytestmark = pytest.mark.gpu

SMALL_NAME, LONG_NAME, NEAR_NAME = "driver_131x513", "driver_1300x1100", "near"
SMALL, LONG, NEAR = (PC.CASES[n][0] for n in (SMALL_NAME, LONG_NAME, NEAR_NAME))
PLANNED = PC.cloud(400, 4099, 5)
PLANNED_SLICES = 3
# second value sets
SMALL_B = PC.cloud(9713, SMALL.n_src, len(SMALL.r_trg))
PLANNED_B = PC.cloud(9005, PLANNED.n_src, len(PLANNED.r_trg))

FIBERS, FIBERS_B = PC.fiber_points(3, 7), PC.fiber_points(3, 7, seed=52)
SURFACE, SURFACE_B = PC.surface_points(7), PC.surface_points(7, seed=160)

TENSORS = ("r_src", "r_trg", "f3", "f9", "nrm")


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


@pytest.fixture(scope="module")
def side():
    """One side stream for the tests that need no more than 'not the default
    one' (torch hands out 32 streams and then the first again)."""
    import torch
    return torch.cuda.Stream()


# the nine device forms by PC.KERNELS name: fn(ska, d, out=None), d from dev()
DEVICE = {
    "stokeslet": lambda ska, d, out=None: ska.stokeslet_device(
        d.r_src, d.f3, d.r_trg, d.eta, out=out),
    "stresslet": lambda ska, d, out=None: ska.stresslet_device(
        d.r_src, d.f9, d.r_trg, d.eta, out=out),
    "oseen": lambda ska, d, out=None: ska.oseen_contract_device(
        d.r_src, d.r_trg, d.f3, d.eta, d.reg, d.eps, out=out),
    "rotlet": lambda ska, d, out=None: ska.rotlet_device(
        d.r_src, d.r_trg, d.f3, d.eta, d.reg, d.eps, out=out),
    "normal_density": lambda ska, d, out=None: ska.stresslet_normal_density_device(
        d.r_src, d.nrm, d.f3, d.r_trg, reg=d.reg, epsilon_distance=d.eps, out=out),
    "stokeslet_grad": lambda ska, d, out=None: ska.stokeslet_grad_device(
        d.r_src, d.f3, d.r_trg, d.eta, out=out),
    "stresslet_grad": lambda ska, d, out=None: ska.stresslet_grad_device(
        d.r_src, d.f9, d.r_trg, d.eta, out=out),
    "oseen_grad": lambda ska, d, out=None: ska.oseen_contract_grad_device(
        d.r_src, d.r_trg, d.f3, d.eta, d.reg, d.eps, out=out),
    "rotlet_grad": lambda ska, d, out=None: ska.rotlet_grad_device(
        d.r_src, d.r_trg, d.f3, d.eta, d.reg, d.eps, out=out),
}
assert list(DEVICE) == PC.KERNELS
# the tensors of dev() that a kernel reads
READS = {k: ("r_src", "r_trg", "f9" if k.startswith("stresslet") else "f3")
         + (("nrm",) if k == "normal_density" else ()) for k in DEVICE}
OUTDIM = {k: 9 if k.endswith("_grad") else 3 for k in DEVICE}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def dev(c):
    """A Case on the device (tensors of its own), the copies complete."""
    import torch
    d = SimpleNamespace(eta=c.eta, reg=c.reg, eps=c.eps,
                        **{name: _t(getattr(c, name)) for name in TENSORS})
    torch.cuda.synchronize()
    return d


def fetch(fn, stream=None):
    """fn()'s tensor as a numpy array: called on `stream` (torch's default
    without one), then everything synchronized."""
    import torch
    if stream is None:
        out = fn()
    else:
        with torch.cuda.stream(stream):
            out = fn()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@contextmanager
def knobs(persistent_ws, slices=0, fastpath=1):
    from skellysim_amd import _native
    lib = _native.lib()
    try:
        lib.skelly_set_persistent_ws(persistent_ws)
        _native.set_pair_slices(slices)
        _native.set_pair_fastpath(fastpath)
        yield lib
    finally:
        lib.skelly_set_persistent_ws(-1)  # the default (on)
        _native.set_pair_slices(0)
        _native.set_pair_fastpath(1)


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), \
        f"{what}: {np.count_nonzero(got != want)} of {want.size} entries differ"


# ---- 1. every device form on a side stream ---------------------------------------

@pytest.mark.parametrize("n_slices", [1, 3])
@pytest.mark.parametrize("kernel", PC.KERNELS)
def test_side_stream_launch_equals_default_stream(ska, side, kernel, n_slices):
    """Fast path on, on again and off, with the mempool workspace and with the
    persistent one: the side-stream result is the default-stream result, and
    inside the kernel's bound."""
    d = dev(SMALL)
    ref, A = PC.reference(SMALL_NAME, kernel, SMALL)
    limit = R.bound(A, SMALL.n_src, n_slices, kernel)
    for ws in (0, 1):
        with knobs(ws):
            plain = sliced(n_slices, lambda: fetch(lambda: DEVICE[kernel](ska, d)))
        with knobs(ws):
            aside = sliced(n_slices, lambda: fetch(lambda: DEVICE[kernel](ska, d), side))
        for mode, a, b in zip(("fastpath on", "on again", "fastpath off"), aside, plain):
            same(a, b, f"{kernel} slices={n_slices} ws={ws} {mode}, side against default stream")
        judge(f"{kernel} {SMALL_NAME} slices={n_slices} side stream ws={ws}", aside[0], ref, A,
              limit)


def _oseen_tensor(ska, pts, out=None):
    return ska.oseen_tensor_batched_device(pts, eta=1.3, out=out)


def _times_normal(ska, pts, nrm, out=None):
    return ska.stresslet_times_normal_device(pts, nrm, out=out)


def test_side_stream_dense_builders(ska, side):
    import torch
    pts, r, nrm = _t(FIBERS), _t(SURFACE.r_src), _t(SURFACE.nrm)
    torch.cuda.synchronize()
    with knobs(0):
        G = fetch(lambda: _oseen_tensor(ska, pts), side)
        same(G, fetch(lambda: _oseen_tensor(ska, pts)), "oseen_tensor on a side stream")
        S = fetch(lambda: _times_normal(ska, r, nrm), side)
        same(S, fetch(lambda: _times_normal(ska, r, nrm)), "stresslet_times_normal, side stream")
    ref, A = R.oseen_tensor_batched(FIBERS, 1.3)
    judge("oseen_tensor 3x7 side stream", G, ref, A, R.entry_bound(A, "oseen_tensor"))
    ref, A = R.stresslet_times_normal(SURFACE.r_src, SURFACE.nrm)
    judge("stresslet_times_normal 7 side stream", S, ref, A,
          R.entry_bound(A, "stresslet_times_normal"))


# ---- 2. stream order is the only order -------------------------------------------

@pytest.mark.parametrize("consumer", ["clone", "sum"])
@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "stokeslet_grad"])
def test_stream_order_is_the_only_order(ska, side, kernel, consumer):
    """The inputs hold NaN until a copy that is queued on the side stream behind
    a few milliseconds of matmuls; the kernel is queued behind the copy and its
    consumer behind the kernel, with no host synchronization anywhere. Stream
    order alone makes the result the synchronous one, so correct code can never
    fail this. A launch that went to another stream (the null stream, say)
    runs while the matmuls still hold the side stream back and reads NaN; that
    wrong code is caught is likely, not certain: it rests on the matmuls
    outlasting the launch latency."""
    import torch
    staged = dev(SMALL)
    with knobs(0):
        want = DEVICE[kernel](ska, staged)
        want = want.sum() if consumer == "sum" else want
        torch.cuda.synchronize()
        want = want.cpu().numpy()
        live = SimpleNamespace(**vars(staged))
        for name in READS[kernel]:
            setattr(live, name, torch.full_like(getattr(staged, name), float("nan")))
        a = torch.randn(2048, 2048, dtype=torch.float64, device="cuda:0") / 64.0
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            b = a
            for _ in range(12):
                b = b @ a
            for name in READS[kernel]:
                getattr(live, name).copy_(getattr(staged, name))
            out = DEVICE[kernel](ska, live)
            got = out.sum() if consumer == "sum" else out.clone()
        torch.cuda.synchronize()
    same(got.cpu().numpy(), want, f"{kernel} behind queued work, {consumer}")


# ---- 3. two streams at once, a workspace per stream ------------------------------

@pytest.mark.parametrize("ws", [1, 0])
def test_two_streams_alternating(ska, side, ws):
    """LONG stresslet on one stream and SMALL rotlet_grad in 3 slices on the
    other, ten times each without a synchronization: with one workspace for
    both streams, a launch's records and partials would be overwritten under
    it."""
    import torch
    from skellysim_amd import _native
    other = torch.cuda.Stream()
    big, small = dev(LONG), dev(SMALL)
    with knobs(ws):
        want_big = fetch(lambda: DEVICE["stresslet"](ska, big))
        _native.set_pair_slices(3)
        want_small = fetch(lambda: DEVICE["rotlet_grad"](ska, small))
        outs = []
        for _ in range(10):
            _native.set_pair_slices(0)
            with torch.cuda.stream(side):
                outs.append(DEVICE["stresslet"](ska, big))
            _native.set_pair_slices(3)
            with torch.cuda.stream(other):
                outs.append(DEVICE["rotlet_grad"](ska, small))
        torch.cuda.synchronize()
    for i, out in enumerate(outs):
        same(out.cpu().numpy(), want_small if i % 2 else want_big, f"ws={ws} launch {i}")


# ---- 4. growth behind queued work ------------------------------------------------

def block_bytes(stream):
    """Capacity of the persistent workspace block the library keeps for a
    torch stream."""
    import ctypes
    from skellysim_amd import _native
    n = ctypes.c_longlong(-1)
    assert _native.lib().skelly_persistent_ws_bytes(ctypes.c_void_p(stream.cuda_stream),
                                                    ctypes.byref(n)) == 0
    return n.value


def outgrowing_slices(stream, outdim):
    """A slice count at which LONG's partials alone exceed the block `stream`
    has now (torch hands out 32 streams and then the first again, so a stream
    new to a test may come with a block)."""
    n = block_bytes(stream) // (8 * outdim * len(LONG.r_trg)) + 2
    assert n <= LONG.n_src, "the stream's block is beyond what LONG can outgrow"
    return n


def test_workspace_growth_behind_queued_work(ska):
    """Five SMALL launches are queued on a stream whose block they fit, then
    LONG in as many slices as do not fit it: the block is replaced while the
    five may still be running out of it, and must stay theirs (retired, not
    freed). The reference runs through the mempool workspace, a fresh one per
    launch."""
    import torch
    from skellysim_amd import _native
    s = torch.cuda.Stream()
    small, big = dev(SMALL), dev(LONG)
    with knobs(1):
        fetch(lambda: DEVICE["stokeslet"](ska, small), s)  # the block SMALL fits
        before = block_bytes(s)
        n_slices = outgrowing_slices(s, 3)
    with knobs(0):
        want = fetch(lambda: DEVICE["stokeslet"](ska, small))
        _native.set_pair_slices(n_slices)
        want_big = fetch(lambda: DEVICE["stokeslet"](ska, big))
    with knobs(1):
        with torch.cuda.stream(s):
            outs = [DEVICE["stokeslet"](ska, small) for _ in range(5)]
            _native.set_pair_slices(n_slices)
            out_big = DEVICE["stokeslet"](ska, big)
            _native.set_pair_slices(0)
            outs.append(DEVICE["stokeslet"](ska, small))
        torch.cuda.synchronize()
        assert block_bytes(s) > before > 0, "the LONG launch did not outgrow the block"
    for i, out in enumerate(outs):
        same(out.cpu().numpy(), want, f"SMALL launch {i}")
    same(out_big.cpu().numpy(), want_big, "LONG launch")


# ---- 5. capture and replay, kernel by kernel -------------------------------------

def _capture_and_check(call, copy_in, forced, check_second, grow):
    """call(): the launch on its static inputs; copy_in(): the second value
    set into them; forced: the slice knob at capture; check_second(out):
    the bound of the second set; grow(s): an eager launch on s that outgrows
    the captured block."""
    import torch
    from skellysim_amd import _native
    s = torch.cuda.Stream()
    with knobs(1, slices=forced):
        eager_first = fetch(call)
        with torch.cuda.stream(s):
            call()
            call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = call()
        # from here on the knob differs from the captured launch's count

        def replay():
            with torch.cuda.stream(s):
                out.fill_(float("nan"))
                g.replay()
            torch.cuda.synchronize()
            return out.cpu().numpy()

        _native.set_pair_slices(0)
        same(replay(), eager_first, "(a) replay of the captured values")
        copy_in()
        torch.cuda.synchronize()
        _native.set_pair_slices(forced)
        eager_second = fetch(call)
        _native.set_pair_slices(0)
        assert not np.array_equal(eager_second, eager_first)
        got = replay()
        same(got, eager_second, "(b) replay after new values were copied in")
        check_second(got)
        for i in range(2):
            same(replay(), got, f"(c) replay {i + 2} of 3")
        captured_against = block_bytes(s)
        grow(s)
        torch.cuda.synchronize()
        _native.set_pair_slices(0)
        assert block_bytes(s) > captured_against, "the eager launch did not outgrow the block"
        same(replay(), eager_second, "(d) replay after the workspace outgrew the captured block")


def _grow_with(ska, kernel):
    """grow(s): LONG through `kernel` on s, in as many slices as s's block
    does not hold."""
    import torch
    from skellysim_amd import _native
    big = dev(LONG)

    def grow(s):
        _native.set_pair_slices(outgrowing_slices(s, OUTDIM[kernel]))
        with torch.cuda.stream(s):
            DEVICE[kernel](ska, big)
    return grow


@pytest.mark.parametrize("shape,forced", [("small", 1), ("small", 3), ("planned", 0)])
@pytest.mark.parametrize("kernel", PC.KERNELS)
def test_captured_launch_replays(ska, kernel, shape, forced):
    """The graph holds the packing of the source records, the slice count it
    was captured with and the block it was captured against: new values in the
    static inputs come out as the eager launch has them, with the slice knob
    back at 0, and after an eager launch on the same stream made the workspace
    grow (observed: the block's capacity is read before and after)."""
    first, second, name = ((SMALL, SMALL_B, "small_b") if shape == "small" else
                           (PLANNED, PLANNED_B, "planned_b"))
    n_slices = forced or PLANNED_SLICES
    static, fresh = dev(first), dev(second)
    ref, A = PC.reference(name, kernel, second)
    limit = R.bound(A, second.n_src, n_slices, kernel)

    def copy_in():
        for t in READS[kernel]:
            getattr(static, t).copy_(getattr(fresh, t))

    _capture_and_check(
        lambda: DEVICE[kernel](ska, static), copy_in, forced,
        lambda got: judge(f"{kernel} {name} slices={forced} replay", got, ref, A, limit),
        _grow_with(ska, kernel))


def test_captured_oseen_tensor_replays(ska):
    pts, fresh = _t(FIBERS), _t(FIBERS_B)
    ref, A = R.oseen_tensor_batched(FIBERS_B, 1.3)
    _capture_and_check(
        lambda: _oseen_tensor(ska, pts), lambda: pts.copy_(fresh), 0,
        lambda got: judge("oseen_tensor 3x7 replay", got, ref, A,
                          R.entry_bound(A, "oseen_tensor")),
        _grow_with(ska, "stokeslet"))


def test_captured_stresslet_times_normal_replays(ska):
    r, nrm = _t(SURFACE.r_src), _t(SURFACE.nrm)
    r_b, nrm_b = _t(SURFACE_B.r_src), _t(SURFACE_B.nrm)
    ref, A = R.stresslet_times_normal(SURFACE_B.r_src, SURFACE_B.nrm)

    def copy_in():
        r.copy_(r_b)
        nrm.copy_(nrm_b)

    _capture_and_check(
        lambda: _times_normal(ska, r, nrm), copy_in, 0,
        lambda got: judge("stresslet_times_normal 7 replay", got, ref, A,
                          R.entry_bound(A, "stresslet_times_normal")),
        _grow_with(ska, "stokeslet"))


# ---- 6. host-layer state ---------------------------------------------------------

def _host_calls(ska):
    """Host-form calls whose rows are 9, 3, 3 and 6 doubles in and 9, 3, 3
    and 3 out, through role buffers that are sized in bytes and only grow."""
    one = PC.CASES["pair_1x257"][0]
    return [
        ("stresslet_grad LONG", lambda: EVALUATE["stresslet_grad"](ska, LONG)),
        ("stokeslet 1x257", lambda: EVALUATE["stokeslet"](ska, one)),
        ("rotlet LONG", lambda: EVALUATE["rotlet"](ska, LONG)),
        ("normal_density NEAR", lambda: ska.stresslet_times_normal_times_density(
            NEAR.r_src, NEAR.nrm, NEAR.f3, NEAR.reg, NEAR.eps)),
    ]


@pytest.fixture(scope="module")
def first_after_shutdown(ska):
    """Each call of _host_calls as the first one after skelly_hip_shutdown():
    into buffers allocated for it."""
    out = {}
    with knobs(0) as lib:
        for what, call in _host_calls(ska):
            assert lib.skelly_hip_shutdown() == 0
            out[what] = call()
            assert np.isfinite(out[what]).all()
    return out


def test_role_buffers_across_row_widths(ska, first_after_shutdown):
    with knobs(0) as lib:
        assert lib.skelly_hip_shutdown() == 0
        for what, call in _host_calls(ska):
            same(call(), first_after_shutdown[what], what + " after the calls before it")


def test_shutdown_and_reuse(ska, first_after_shutdown):
    with knobs(0) as lib:
        for what, call in _host_calls(ska):
            call()
        assert lib.skelly_hip_shutdown() == 0
        assert lib.skelly_hip_shutdown() == 0
        for what, call in _host_calls(ska):
            same(call(), first_after_shutdown[what], what + " after shutdown")


def test_two_threads_are_serialized(ska):
    """Ten host calls on each of two threads (ctypes releases the GIL, so they
    do meet in the library): one set of role buffers and one stream, and only
    the mutex between them."""
    jobs = {
        "a": [lambda: EVALUATE["stresslet"](ska, LONG)],
        "b": [lambda: EVALUATE["stokeslet_grad"](ska, SMALL),
              lambda: EVALUATE["oseen"](ska, NEAR)],
    }
    got = {k: [] for k in jobs}

    def work(k, lib):
        try:
            for i in range(10):
                got[k].append(jobs[k][i % len(jobs[k])]())
            got[k].append(lib.skelly_hip_last_error().decode())
        except BaseException as e:  # reported by the asserts below
            got[k].append(e)

    with knobs(0) as lib:
        want = {k: [call() for call in calls] for k, calls in jobs.items()}
        threads = [threading.Thread(target=work, args=(k, lib)) for k in jobs]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    for k in jobs:
        assert len(got[k]) == 11 and got[k][-1] == "", got[k][-1]
        for i, u in enumerate(got[k][:10]):
            same(u, want[k][i % len(want[k])], f"thread {k} call {i}")


# ---- 7. device-tensor arguments --------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    """_native.lib raises: whatever the validation does, nothing is launched."""
    from skellysim_amd import _native

    def lib():
        raise AssertionError("reached the library")
    monkeypatch.setattr(_native, "lib", lib)


def _z(*shape, **kw):
    import torch
    kw.setdefault("dtype", torch.float64)
    kw.setdefault("device", "cuda:0")
    return torch.zeros(shape, **kw)


@pytest.mark.parametrize("n_f", [9, 11])
def test_device_forms_reject_strengths_of_another_length(ska, no_library, n_f):
    with pytest.raises(ValueError, match="f_src"):
        ska.stokeslet_device(_z(10, 3), _z(n_f, 3), _z(4, 3), 1.3)
    with pytest.raises(ValueError, match="f_src"):
        ska.stresslet_grad_device(_z(10, 3), _z(n_f, 9), _z(4, 3), 1.3)
    with pytest.raises(ValueError, match="density"):
        ska.rotlet_device(_z(10, 3), _z(4, 3), _z(n_f, 3))
    with pytest.raises(ValueError, match="density"):
        ska.oseen_contract_grad_device(_z(10, 3), _z(4, 3), _z(n_f, 3))
    with pytest.raises(ValueError, match="normals"):
        ska.stresslet_normal_density_device(_z(10, 3), _z(n_f, 3), _z(10, 3))
    with pytest.raises(ValueError, match="density"):
        ska.stresslet_normal_density_device(_z(10, 3), _z(10, 3), _z(n_f, 3), _z(4, 3))
    with pytest.raises(ValueError, match="normals"):
        ska.stresslet_times_normal_device(_z(10, 3), _z(n_f, 3))


def _bad_outs(*shape):
    import torch
    numel = int(np.prod(shape))
    strided = _z(*shape[:-1], 2 * shape[-1])[..., ::2]
    assert strided.numel() == numel and not strided.is_contiguous()
    return {
        "too small": _z(numel - 1),
        "too large": _z(numel + 1),
        "float32": _z(*shape, dtype=torch.float32),
        "non-contiguous": strided,
        "on the CPU": _z(*shape, device="cpu"),
        "no tensor": np.zeros(shape),
    }


def test_dense_builders_reject_an_out_they_cannot_write(ska, no_library):
    for what, out in _bad_outs(21, 21).items():
        with pytest.raises(ValueError, match="out"):
            ska.stresslet_times_normal_device(_z(7, 3), _z(7, 3), out=out)
    for what, out in _bad_outs(3, 21, 21).items():
        with pytest.raises(ValueError, match="out"):
            ska.oseen_tensor_batched_device(_z(3, 7, 3), out=out)
    for what, out in _bad_outs(4, 3).items():
        with pytest.raises(ValueError, match="out"):
            ska.stokeslet_device(_z(10, 3), _z(10, 3), _z(4, 3), 1.3, out=out)


def test_valid_out_is_filled_and_returned(ska):
    import torch
    pts, r, nrm = _t(FIBERS), _t(SURFACE.r_src), _t(SURFACE.nrm)
    d = dev(SMALL)
    with knobs(0):
        for what, call, shape in (
                ("oseen_tensor", lambda out=None: _oseen_tensor(ska, pts, out), (3, 21, 21)),
                ("stresslet_times_normal", lambda out=None: _times_normal(ska, r, nrm, out),
                 (21, 21)),
                ("stokeslet_grad", lambda out=None: DEVICE["stokeslet_grad"](ska, d, out),
                 (len(SMALL.r_trg), 3, 3))):
            want = fetch(call)
            out = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")
            assert call(out) is out, what
            torch.cuda.synchronize()
            same(out.cpu().numpy(), want, what + " into out=")
