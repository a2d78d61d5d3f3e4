"""The streamline tracer without a GPU: the stepper and its control law as
tests/streamline_reference.py restates them (the reference of
tests/test_gpu_streamlines.py), the argument contract of the two C entry
points, the joining of the per-job arrays, and the preconditions under which
the GPU comparison means something, checked here on the reference alone."""

import ctypes
import threading
from fractions import Fraction as Fr

import numpy as np
import pytest

import streamline_reference as S
from skellysim_amd import _native


# ---- the tableau ------------------------------------------------------------------

def test_tableau_rows_sum_to_the_nodes_and_weights_to_one():
    for c, row in zip(S.C, S.A):
        assert sum(row, Fr(0)) == c
    assert sum(S.B5) == 1 and sum(S.B4) == 1


def test_tableau_weights_meet_the_order_conditions():
    """sum b_i c_i^k = 1/(k + 1) up to k = 4 for the 5th-order weights, up to
    k = 3 for the embedded 4th-order ones."""
    for k in range(1, 5):
        assert sum(b * c ** k for b, c in zip(S.B5, S.C)) == Fr(1, k + 1)
    for k in range(1, 4):
        assert sum(b * c ** k for b, c in zip(S.B4, S.C)) == Fr(1, k + 1)


def _rotate(n_steps, t_end=1.0):
    w = np.array([0.3, -0.5, 0.8])
    f = lambda x: np.cross(w, x)
    x = np.array([1.0, 0.2, -0.4])
    x0, dt = x.copy(), t_end / n_steps
    for _ in range(n_steps):
        x, _, _ = S.ck_step(f, x, dt, f(x))
    th = np.linalg.norm(w) * t_end
    k = w / np.linalg.norm(w)
    exact = x0 * np.cos(th) + np.cross(k, x0) * np.sin(th) + k * (k @ x0) * (1 - np.cos(th))
    return np.linalg.norm(x - exact)


def test_fixed_steps_converge_at_fifth_order():
    """x' = w x x: halving the step divides the error by about 2^5."""
    ratio = _rotate(4) / _rotate(8)
    assert 24.0 < ratio < 40.0, ratio


# ---- the law ----------------------------------------------------------------------

def test_rejection_shrinks_by_the_cube_root_floored_at_a_fifth():
    assert S.shrink(2.0) == 0.9 * 2.0 ** (-1.0 / 3.0)
    assert S.shrink(90.0) > 0.2 and S.shrink(92.0) == 0.2  # 0.9 * 91.125^(-1/3) = 0.2
    assert S.shrink(1e30) == 0.2


def test_growth_is_capped():
    assert S.grow(0.4) == 0.9 * 0.4 ** -0.2
    assert S.grow(0.0) == S.grow(1e-30) == pytest.approx(0.9 * 5.0, rel=1e-15)
    assert S.grow(0.0) <= 5.0


def test_a_rejected_try_is_retried_and_growth_follows_a_small_error():
    """A field that bends: the first try at dt = 1 fails, and every accepted
    try follows the law's dt."""
    f = lambda x: np.array([1.0, np.cos(6.0 * x[0]), -np.sin(4.0 * x[0])])
    r = S.trace(f, [0.0, 0.0, 0.0], dt_init=1.0, t_final=2.0)
    assert r["status"] == S.DONE and not r["accepted"][0] and r["accepted"].any()
    assert (r["errs"][~r["accepted"]] > 1.0).all() and (r["errs"][r["accepted"]] <= 1.0).all()
    # replay dt through the tries
    dt, t, k = 1.0, 0.0, 0
    for err, ok in zip(r["errs"], r["accepted"]):
        if t + dt - 2.0 > S.EPS:
            dt = 2.0 - t
        if not ok:
            dt *= S.shrink(err)
            continue
        t, k = t + dt, k + 1
        assert t == r["t"][k]
        if err < 0.5:
            dt *= S.grow(err)


@pytest.mark.parametrize("t_final", [1.0, -1.0])
def test_last_step_is_clipped_onto_t_final(t_final):
    r = S.trace(lambda x: np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0], dt_init=0.3,
                t_final=t_final)
    assert r["status"] == S.DONE
    assert r["t"][-1] == t_final and r["t"][0] == 0.0
    assert np.all(np.diff(r["t"]) * np.sign(t_final) > 0)
    assert r["x"][-1, 0] == pytest.approx(t_final, abs=1e-15)


def test_singular_point_is_recorded_before_the_stop():
    f = lambda x: np.array([2e3, 0.0, 0.0])
    r = S.trace(f, [0.1, 0.2, 0.3])
    assert r["status"] == S.SINGULAR and r["count"] == 1
    assert np.array_equal(r["x"], [[0.1, 0.2, 0.3]]) and np.array_equal(r["val"], [[2e3, 0, 0]])
    assert len(r["errs"]) == 0


def test_capacity_stop():
    f = lambda x: np.array([1.0, np.cos(6.0 * x[0]), 0.0])
    full = S.trace(f, [0.0, 0.0, 0.0], dt_init=0.01, t_final=5.0)
    assert full["status"] == S.DONE and full["count"] > 4
    r = S.trace(f, [0.0, 0.0, 0.0], dt_init=0.01, t_final=5.0, max_points=4)
    assert r["status"] == S.FULL and r["count"] == 4
    assert np.array_equal(r["x"], full["x"][:4])
    exact = S.trace(f, [0.0, 0.0, 0.0], dt_init=0.01, t_final=5.0, max_points=full["count"])
    assert exact["status"] == S.DONE and exact["count"] == full["count"]


def test_a_step_that_cannot_pass_gives_up():
    """A NaN field: no try has err <= 1, dt shrinks until it no longer moves t."""
    r = S.trace(lambda x: np.full(3, np.nan), [0.0, 0.0, 0.0], max_points=8)
    assert r["status"] == S.GAVE_UP and r["count"] == 1
    assert not r["accepted"].any() and len(r["errs"]) < 1000


# ---- joining ----------------------------------------------------------------------

def test_join_reverses_the_backward_path_and_drops_its_seed():
    from skellysim_amd.evaluator import join_streamlines
    n, cap = 2, 5
    x = np.arange(4 * cap * 3, dtype=float).reshape(4, cap, 3)
    t = np.arange(4 * cap, dtype=float).reshape(4, cap)
    count, status = np.array([3, 2, 4, 1]), np.array([0, 2, 1, 0])
    lines = join_streamlines(x, t, x + 0.5, count, status, n)
    assert np.array_equal(lines[0]["time"], [t[2, 3], t[2, 2], t[2, 1], t[0, 0], t[0, 1], t[0, 2]])
    assert np.array_equal(lines[0]["x"][:3], x[2, 3:0:-1]) and lines[0]["status"] == 1
    assert np.array_equal(lines[0]["val"], lines[0]["x"] + 0.5)
    assert np.array_equal(lines[1]["time"], t[1, :2]) and lines[1]["status"] == 2
    forward = join_streamlines(x[:2], t[:2], x[:2], count[:2], status[:2], n)
    assert np.array_equal(forward[0]["x"], x[0, :3]) and forward[0]["status"] == 0


# ---- the C boundary ---------------------------------------------------------------

ENTRY_POINTS = ["skelly_trace_streamlines_host", "skelly_trace_streamlines_device"]


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


def _n_counts(name):
    return sum(t is _native.TraceCount for t in _native.SIGNATURES[name][1])


def test_streamline_entry_points_keep_their_own_count_type():
    """Seven counts each (four sets, bodies, seeds, max_points), none of them a
    plain c_longlong, by which tests/test_evaluator_arguments.py enumerates."""
    for name in ENTRY_POINTS:
        argtypes = _native.SIGNATURES[name][1]
        assert _n_counts(name) == 7
        assert not any(t is ctypes.c_longlong for t in argtypes)
    assert issubclass(_native.TraceCount, ctypes.c_longlong)


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


# ---- preconditions of the GPU comparison ------------------------------------------

def test_mixed_cloud_is_the_one_the_comparison_is_specified_on():
    c = S.mixed_cloud()
    rng = np.random.default_rng(100)
    assert np.array_equal(c["stokeslet"][0], rng.uniform(-1, 1, (301, 3)))
    assert np.array_equal(c["stokeslet"][1], rng.uniform(-1, 1, (301, 3)))
    assert np.array_equal(c["rotlet"][0], rng.uniform(-1, 1, (5, 3)))
    assert np.array_equal(c["rotlet"][1], rng.uniform(-1, 1, (5, 3)))
    assert np.array_equal(c["seeds"], rng.uniform(-1, 1, (7, 3)))
    assert c["stresslet"][1].shape == (97, 9) and c["oseen"][0].shape == (3, 3)


def test_enough_seeds_remain():
    assert len(S.kept_seeds()) >= 5
    assert set(S.DROPPED) <= set(range(7))


def test_precondition_a_no_decision_sits_on_its_threshold(oracle_mod):
    """Every try's err of every kept run keeps a relative distance of 1e-4
    from 1 (accept or reject) and from 0.5 (grow or not)."""
    for i, tf, run in S.mixed_reference():
        margin = S.threshold_margin(run)
        print(f"seed {i} t_final {tf:+.0f}: {run['count']} points, status {run['status']}, "
              f"{len(run['errs'])} tries, margin {margin:.2e}")
        if i not in S.DROPPED:
            assert margin >= 1e-4, (i, tf, margin)


def test_precondition_b_rounding_size_changes_of_u_leave_the_runs_alone(oracle_mod):
    """With every velocity multiplied by 1 + 1e-13 xi the kept runs keep their
    point count and status, end within 1e-11 and record times within 1e-7.
    (Intermediate points sit at slightly different times and differ by more,
    which is why nothing compares them one by one.)"""
    for (i, tf, run), (_, _, other) in zip(S.mixed_reference(), S.mixed_perturbed()):
        if i in S.DROPPED:
            continue
        assert other["count"] == run["count"] and other["status"] == run["status"], (i, tf)
        end = np.abs(other["x"][-1] - run["x"][-1]).max()
        times = np.abs(other["t"] - run["t"]).max()
        print(f"seed {i} t_final {tf:+.0f}: end {end:.1e}, times {times:.1e}")
        assert end <= 1e-11 and times <= 1e-7, (i, tf, end, times)


def test_mixed_reference_covers_both_ends(oracle_mod):
    """Runs that reach t_final and runs that stop at a singularity, rejected
    tries and accepted ones, more than one point everywhere."""
    runs = [r for i, _, r in S.mixed_reference() if i not in S.DROPPED]
    assert {r["status"] for r in runs} == {S.DONE, S.SINGULAR}
    assert all(r["count"] >= 2 for r in runs)
    assert any((~r["accepted"]).any() for r in runs)
