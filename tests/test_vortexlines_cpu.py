"""The vortex-line tracer without a GPU: the reference of
tests/test_gpu_vortexlines.py (tests/vortexline_reference.py) against the
streamline reference it extends, the preconditions under which the GPU
comparison means something, the case that tells a stop on the velocity from a
stop on the vorticity, and the argument contract of the two C entry points."""

import ctypes
import threading

import numpy as np
import pytest

import streamline_reference as S
import vortexline_reference as V
from skellysim_amd import _native


# ---- the tracer -------------------------------------------------------------------

@pytest.mark.parametrize("t_final", [2.0, -2.0])
def test_trace_with_one_field_is_the_streamline_trace(t_final):
    """rhs is stop: every array of the run equals streamline_reference.trace's,
    rejected tries and a capacity stop included."""
    f = lambda x: np.array([1.0, np.cos(6.0 * x[0]), -np.sin(4.0 * x[0])])
    for cap in (4096, 4):
        a = S.trace(f, [0.0, 0.1, 0.0], dt_init=1.0, t_final=t_final, max_points=cap)
        b = V.trace(f, f, [0.0, 0.1, 0.0], dt_init=1.0, t_final=t_final, max_points=cap)
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), key
        assert a["status"] == (S.FULL if cap == 4 else S.DONE)
        assert cap == 4 or not a["accepted"].all()


def test_singular_stop_reads_the_stop_field_and_records_the_rhs():
    rhs = lambda x: np.array([1.0, 0.0, 0.0])
    r = V.trace(rhs, lambda x: np.array([0.0, 2e3, 0.0]), [0.1, 0.2, 0.3])
    assert r["status"] == V.SINGULAR and r["count"] == 1
    assert np.array_equal(r["val"], [[1.0, 0.0, 0.0]])
    r = V.trace(lambda x: np.array([2e3, 0.0, 0.0]), lambda x: np.zeros(3), [0.1, 0.2, 0.3],
                t_final=1e-3)
    assert r["status"] == V.DONE and r["x"][-1, 0] == pytest.approx(0.1 + 2.0, rel=1e-14)


# ---- the vorticity ----------------------------------------------------------------

def test_background_curl_of_a_rotation():
    W = 0.7
    bg = ((0.0, 0.0, 0.0), (-W, W, 0.0), (1, 0, 2))
    assert np.array_equal(V.background_curl(bg), [0.0, 0.0, 2 * W])
    assert np.array_equal(V.background_curl(S.BACKGROUND), [0.2, -0.1, -0.3])


def test_cloud_vorticity_is_the_central_difference_of_the_oracle_velocity(oracle_mod):
    """The analytic curl against the curl of the oracle's velocity by central
    differences, at the seeds of the mixed cloud."""
    w, u = V.mixed_fields()
    x = S.mixed_cloud()["seeds"]
    omega, A = w(x)
    h = 1e-5
    G = np.zeros((len(x), 3, 3))
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        G[:, :, j] = (u(x + e) - u(x - e)) / (2 * h)
    fd = V.curl(G)
    assert np.abs(fd - np.asarray(omega, float)).max() <= 1e-6 * np.asarray(A, float).max()


def test_inside_a_body_the_vorticity_is_twice_the_angular_velocity():
    bodies = np.array([[0, 0, 0, 1.0, 1, 2, 3, 0.1, 0.2, 0.3],
                       [0.1, 0, 0, 0.5, 0, 0, 0, -0.4, 0.5, 0.6]])
    w = V.cloud_vorticity(1.0, stokeslet=(np.array([[3.0, 0, 0]]), np.ones((1, 3))),
                          bodies=bodies)
    omega, A = w(np.array([[0.2, 0.0, 0.0], [0.8, 0.0, 0.0], [2.0, 0.0, 0.0]]))
    assert np.array_equal(omega[0], 2 * bodies[1, 7:]) and np.array_equal(omega[1], 2 * bodies[0, 7:])
    assert (A[:2] == 0).all() and (A[2] > 0).any()


# ---- preconditions of the GPU comparison ------------------------------------------

def test_enough_seeds_remain():
    assert len(V.kept_seeds()) >= 5
    assert set(V.DROPPED) <= set(range(7))


def test_mixed_runs_finish_in_a_small_buffer(oracle_mod):
    runs = [r for i, _, r in V.mixed_reference() if i not in V.DROPPED]
    assert all(r["status"] == V.DONE for r in runs)
    assert all(2 <= r["count"] < 130 for r in runs)
    assert any((~r["accepted"]).any() for r in runs)


def test_precondition_a_no_decision_sits_on_its_threshold(oracle_mod):
    """Every try's err of every kept run keeps a relative distance of 1e-4
    from 1 (accept or reject) and from 0.5 (grow or not)."""
    for i, tf, run in V.mixed_reference():
        margin = S.threshold_margin(run)
        print(f"seed {i} t_final {tf:+.0f}: {run['count']} points, status {run['status']}, "
              f"{len(run['errs'])} tries, margin {margin:.2e}")
        if i not in V.DROPPED:
            assert margin >= 1e-4, (i, tf, margin)


def test_precondition_b_bound_size_changes_of_the_vorticity_leave_the_runs_alone(oracle_mod):
    """With 2e-13 A_omega xi added to every vorticity component the kept runs
    keep their point count and status, end within 1e-11 and record times within
    2e-7 (measured: 1.8e-12 and 6.0e-8; at ten times the amplitude 1.7e-11 and
    6.0e-7, so the response is linear)."""
    for (i, tf, run), (_, _, other) in zip(V.mixed_reference(), V.mixed_perturbed()):
        if i in V.DROPPED:
            continue
        assert other["count"] == run["count"] and other["status"] == run["status"], (i, tf)
        end = np.abs(other["x"][-1] - run["x"][-1]).max()
        times = np.abs(other["t"] - run["t"]).max()
        print(f"seed {i} t_final {tf:+.0f}: end {end:.1e}, times {times:.1e}")
        assert end <= 1e-11 and times <= 2e-7, (i, tf, end, times)


# ---- the stop is on the velocity --------------------------------------------------

def test_a_large_vorticity_beside_a_moderate_velocity_does_not_stop_the_line(oracle_mod):
    w, u = V.near_fields()
    seed = V.NEAR["seed"]
    assert np.linalg.norm(V.as_rhs(w)(seed)) > 1e3 > np.linalg.norm(u(seed))
    run = V.near_reference()
    assert run["status"] == V.DONE and run["count"] < 130
    assert abs(run["t"][-1] - V.NEAR["t_final"]) <= V.EPS
    assert S.threshold_margin(run) >= 1e-4
    # the same line under the streamline rule (stop on the integrated field)
    rhs = V.as_rhs(w)
    stopped = V.trace(rhs, rhs, seed, V.NEAR["dt_init"], V.NEAR["t_final"])
    assert stopped["status"] == V.SINGULAR and stopped["count"] == 1


# ---- the C boundary ---------------------------------------------------------------

ENTRY_POINTS = ["skelly_trace_vortexlines_host", "skelly_trace_vortexlines_device"]


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    so = ctypes.CDLL(hip_lib_path)
    _native._bind(so)
    return so


def _call(lib, name, counts):
    """(rc, message) of one call with null pointers and `counts` in the count
    positions, on a thread of its own (the message is per thread)."""
    counts = iter(counts)
    args = [next(counts) if t is _native.TraceCount else 1e-3 if t is ctypes.c_double
            else 1 if t is ctypes.c_int else None for t in _native.SIGNATURES[name][1]]
    got = []

    def run():
        got.append(getattr(lib, name)(*args))
        got.append(lib.skelly_hip_last_error().decode())
    th = threading.Thread(target=run)
    th.start()
    th.join()
    return got


def test_vortexline_entry_points_take_the_streamline_arguments():
    """The argument lists of the streamline entry points: seven TraceCount
    counts each, none of them a plain c_longlong."""
    for name in ENTRY_POINTS:
        restype, argtypes = _native.SIGNATURES[name]
        assert (restype, argtypes) == _native.SIGNATURES[name.replace("vortex", "stream")]
        assert sum(t is _native.TraceCount for t in argtypes) == 7
        assert not any(t is ctypes.c_longlong for t in argtypes)


@pytest.mark.parametrize("bad", range(7))
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_negative_count_is_an_error_before_any_launch(lib, name, bad):
    for value in (-1, -(1 << 40)):
        rc, msg = _call(lib, name, [value if i == bad else 5 for i in range(7)])
        assert rc != 0
        assert msg.startswith(name + ":") and "negative" in msg, msg


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_zero_seeds_is_no_error_and_touches_nothing(lib, name):
    rc, msg = _call(lib, name, [5, 5, 5, 5, 5, 0, 5])
    assert rc == 0 and msg == ""
