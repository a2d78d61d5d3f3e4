"""The device vortex-line tracer against the CPU reference of
tests/vortexline_reference.py, and the layers above it.

The comparison is on the mixed cloud of tests/streamline_reference.py at
eta = 64 (vortexline_reference says why), 7 seeds both ways. As for the
streamlines, points are not compared one by one: a change of the vorticity of
the rounding bound's size moves the step sizes and with them the times of the
intermediate points (tests/test_vortexlines_cpu.py, precondition (b)). What
is compared is what that precondition shows to be stable: count, status, end
point and times; `val` is held to the pair kernels' rounding bound at every
recorded point, and every recorded step is replayed on its own with reference
vorticities, which holds each intermediate point to the stepper."""

import os
import shutil
import subprocess

import msgpack
import numpy as np
import pytest

import pair_reference as P
import streamline_reference as S
import vortexline_reference as V
from test_gpu_streamlines import (X0, _block_bytes, _request, _serve, _sources, _WithSets,
                                  job_rows, same_jobs)
from test_gpu_streamlines import backend, trajectory  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS = V.MAX_POINTS  # the longest reference run of the mixed cloud has 27 points


def trace_mixed(backend, seeds=None, **kw):
    c = S.mixed_cloud()
    kw = dict(dict(dt_init=V.DT_INIT, t_final=V.T_FINAL, back_integrate=True,
                   max_points=MAX_POINTS), **kw)
    return backend.trace_vortexlines(c["seeds"] if seeds is None else seeds, V.ETA,
                                     **S.mixed_sets(c), **kw)


@pytest.fixture(scope="module")
def mixed(backend):
    return trace_mixed(backend)


def cloud_extent(c, keys):
    pts = np.concatenate([c[k][0] for k in keys] + [c["seeds"]])
    return float(np.max(pts.max(axis=0) - pts.min(axis=0)))


def assert_matches(out, j, ref, seed, tf, extent, what):
    """Test 1's comparison of job j with its reference run."""
    x, t, val, count, status = job_rows(out, j)
    end = np.abs(x[-1] - ref["x"][-1]).max() if count == ref["count"] else np.nan
    times = np.abs(t - ref["t"]).max() if count == ref["count"] else np.nan
    print(f"{what} t_final {tf:+.0f}: count {count} ({ref['count']}), status {status} "
          f"({ref['status']}), end {end:.2e}, times {times:.2e}")
    assert (status, count) == (ref["status"], ref["count"]), (what, tf)
    assert end <= 1e-10 * extent, (what, tf, end)
    assert times <= 2e-6, (what, tf, times)
    assert t[0] == 0.0 and np.array_equal(x[0], seed)
    if status == V.DONE:
        assert abs(t[-1] - tf) <= V.EPS  # the loop's own exit condition


def assert_val_is_the_vorticity(w, x, val, background, what):
    """Test 2's bound at the points x, per component."""
    omega, A = w(x)
    bound = V.val_bound(w, x, background)
    err = np.abs(np.asarray(val, P.LD) - omega)
    exact = np.asarray(A) == 0
    assert np.array_equal(val[exact], np.asarray(omega, float)[exact]), what
    assert (err <= bound).all(), (what, float((err[~exact] / bound[~exact]).max()))
    return float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0


# ---- 1. the mixed cloud against the reference ---------------------------------------

def test_mixed_cloud_matches_the_reference(oracle_mod, mixed):
    c = S.mixed_cloud()
    extent = cloud_extent(c, ("stokeslet", "stresslet", "rotlet", "oseen"))
    assert (mixed["count"] >= 0).all(), "a job never ran"
    kept = V.kept_seeds()
    assert len(kept) >= 5
    for j, (i, tf, ref) in enumerate(V.mixed_reference()):
        if i in kept:
            assert_matches(mixed, j, ref, c["seeds"][i], tf, extent, f"seed {i}")


# ---- 2. val is the vorticity --------------------------------------------------------

def test_mixed_cloud_val_is_the_vorticity(mixed):
    w = V.cloud_vorticity(V.ETA, **S.mixed_sets())
    worst = 0.0
    for j in range(len(mixed["count"])):
        x, _, val, _, _ = job_rows(mixed, j)
        worst = max(worst, assert_val_is_the_vorticity(w, x, val, S.BACKGROUND, f"job {j}"))
    print(f"val against the longdouble vorticity: worst {worst:.3f} of its bound")


# ---- 3. step replay -----------------------------------------------------------------

def test_mixed_cloud_steps_replay(mixed):
    """From each recorded (x_k, t_{k+1} - t_k) one Cash-Karp step with
    reference vorticities lands on x_{k+1} within 1e-10 |dt| max|k_i| plus
    4 ulp of |x|, and has err <= 1 (it was an accepted step)."""
    f = V.as_rhs(V.cloud_vorticity(V.ETA, **S.mixed_sets()))
    worst = 0.0
    for j in range(len(mixed["count"])):
        x, t, _, count, _ = job_rows(mixed, j)
        for k in range(count - 1):
            dt = t[k + 1] - t[k]
            k1 = f(x[k])
            x5, d, stages = S.ck_step(f, x[k], dt, k1)
            off = np.abs(x5 - x[k + 1]).max()
            bound = 1e-10 * abs(dt) * np.abs(stages).max() + \
                4 * np.finfo(float).eps * np.abs(x[k + 1]).max()
            worst = max(worst, off / bound)
            assert off <= bound, (j, k, off, bound)
            assert S.error_ratio(x[k], dt, k1, d, 1e-10, 1e-6) <= 1.0, (j, k)
    print(f"step replay: worst miss {worst:.2e} of its bound")


# ---- 4. constant curl ---------------------------------------------------------------

W = 2.0
SEED = np.array([[0.7, -0.2, 0.3]])
SPIN = np.array([0.1, -0.2, 0.3])


@pytest.mark.parametrize("how", ["background", "body"])
def test_constant_curl(backend, oracle_mod, how):
    """The rotation (-W y, W x, 0) as the background term, and a seed inside
    two nested bodies whose whole path stays inside both, the later one
    deciding: the vorticity is the constant 2 w and the line x0 + 2 w t."""
    if how == "background":
        field, two_w = dict(background=((0.0, 0.0, 0.0), (-W, W, 0.0), (1, 0, 2))), [0, 0, 2 * W]
    else:
        field = dict(bodies=np.array([[0.0, 0.0, 0.0, 9.0, 3.0, 3.0, 3.0, 1.0, 1.0, 1.0],
                                      [0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, *SPIN]]))
        two_w = 2.0 * SPIN
    two_w = np.asarray(two_w, float)
    out = backend.trace_vortexlines(SEED, 1.0, **field, max_points=MAX_POINTS)
    w = V.cloud_vorticity(1.0, **field)
    u = S.cloud_field(oracle_mod, 1.0, **field)
    for j, tf in enumerate((1.0, -1.0)):
        ref = V.trace(V.as_rhs(w), u, SEED[0], 0.1, tf)
        x, t, val, count, status = job_rows(out, j)
        off = np.abs(x[-1] - (SEED[0] + two_w * tf)).max()
        print(f"{how} t_final {tf:+.0f}: {count} points, end {off:.2e} from x0 + 2 w t")
        assert (status, count) == (V.DONE, ref["count"]) and abs(t[-1] - tf) <= V.EPS
        tol = 1e-14 * (1 + np.linalg.norm(two_w))
        assert off <= tol
        assert np.abs(x - (SEED[0] + two_w * t[:, None])).max() <= tol
        assert np.array_equal(val, np.broadcast_to(two_w, val.shape))


# ---- 5. statuses --------------------------------------------------------------------

def test_strong_stokeslet_is_a_singularity(backend, oracle_mod):
    sl = (np.array([[0.0, 0.0, 0.0]]), np.array([[1e6, 0.0, 0.0]]))
    seed = np.array([[0.1, 0.05, 0.0]])
    out = backend.trace_vortexlines(seed, 1.0, stokeslet=sl, max_points=MAX_POINTS)
    assert np.linalg.norm(oracle_mod.stokeslet(sl[0], sl[1], seed, 1.0)) > 1e3
    w = V.cloud_vorticity(1.0, stokeslet=sl)
    for j in range(2):
        x, t, val, count, status = job_rows(out, j)
        assert (status, count) == (V.SINGULAR, 1)
        assert np.array_equal(x, seed) and t[0] == 0.0
        assert_val_is_the_vorticity(w, x, val, None, f"job {j}")


def test_a_large_vorticity_does_not_stop_the_line(backend, oracle_mod):
    """tests/test_vortexlines_cpu.py's case of |omega| > 1e3 > |u| at the seed:
    the stop is on the velocity, so the line runs as the reference's does."""
    ref = V.near_reference()
    assert ref["status"] == V.DONE and ref["count"] > 1
    out = backend.trace_vortexlines(V.NEAR["seed"][None, :], V.NEAR["eta"],
                                    stokeslet=V.NEAR["stokeslet"], dt_init=V.NEAR["dt_init"],
                                    t_final=V.NEAR["t_final"], back_integrate=False,
                                    max_points=MAX_POINTS)
    x, t, val, count, status = job_rows(out, 0)
    print(f"count {count} ({ref['count']}), status {status} ({ref['status']})")
    assert np.linalg.norm(val[0]) > 1e3
    assert (status, count) == (ref["status"], ref["count"])
    assert abs(t[-1] - V.NEAR["t_final"]) <= V.EPS


def test_full_buffer(backend, mixed):
    out = trace_mixed(backend, max_points=4)
    long_jobs = [j for j in range(len(mixed["count"])) if mixed["count"][j] > 4]
    assert long_jobs
    for j in range(len(mixed["count"])):
        if j in long_jobs:
            assert (int(out["count"][j]), int(out["status"][j])) == (4, V.FULL)
            assert np.array_equal(out["x"][j], mixed["x"][j, :4])
            assert np.array_equal(out["t"][j], mixed["t"][j, :4])
            assert np.array_equal(out["val"][j], mixed["val"][j, :4])
        else:
            same_jobs(out, j, mixed, j, f"job {j} that fits 4 points")


# ---- 6. empty sets ------------------------------------------------------------------

def test_empty_sets(backend, oracle_mod):
    """Stokeslets and rotlets alone (no stresslet, no oseen, no background), at
    eta = 64: against the reference as the mixed cloud is."""
    c = S.mixed_cloud()
    sets = dict(stokeslet=c["stokeslet"], rotlet=c["rotlet"])
    seeds = c["seeds"][:2]
    out = backend.trace_vortexlines(seeds, V.ETA, **sets, stresslet=None,
                                    oseen=(np.zeros((0, 3)), np.zeros((0, 3))),
                                    max_points=MAX_POINTS)
    w, u = V.cloud_vorticity(V.ETA, **sets), S.cloud_field(oracle_mod, V.ETA, **sets)
    extent = cloud_extent(c, ("stokeslet", "rotlet"))
    for j, (i, tf) in enumerate([(0, 1.0), (1, 1.0), (0, -1.0), (1, -1.0)]):
        ref = V.trace(V.as_rhs(w), u, seeds[i], 0.1, tf, max_points=MAX_POINTS)
        assert_matches(out, j, ref, seeds[i], tf, extent, f"seed {i}, two sets")
        x, _, val, _, _ = job_rows(out, j)
        assert_val_is_the_vorticity(w, x, val, None, f"job {j}, two sets")


def test_no_sources_at_all(backend):
    """A uniform background has no curl: every job records the seed at t = 0
    and at t_final, and nothing moves."""
    out = backend.trace_vortexlines(SEED, 1.0, background=((0.5, 0.0, 0.0), (0, 0, 0), (0, 1, 2)),
                                    max_points=MAX_POINTS)
    for j, tf in enumerate((1.0, -1.0)):
        x, t, val, count, status = job_rows(out, j)
        assert status == V.DONE and count >= 2
        assert t[0] == 0.0 and abs(t[-1] - tf) <= V.EPS
        assert np.array_equal(x, np.broadcast_to(SEED[0], x.shape)) and not val.any()


def test_zero_seeds(backend):
    from skellysim_amd.flows import vortexlines_at_seeds
    out = backend.trace_vortexlines(np.zeros((0, 3)), 1.0, **S.mixed_sets())
    assert out["count"].shape == (0,) and out["x"].shape[0] == 0
    assert vortexlines_at_seeds(np.zeros((0, 3)), 1.0, backend=backend) == []


# ---- 7. determinism -----------------------------------------------------------------

def test_two_calls_are_bitwise_equal(backend, mixed):
    again = trace_mixed(backend)
    for j in range(len(mixed["count"])):
        same_jobs(again, j, mixed, j, f"job {j} of a second call")


def test_a_seed_alone_equals_the_seed_among_seven(backend, mixed):
    seeds = S.mixed_cloud()["seeds"]
    for i in (0, 6):
        alone = trace_mixed(backend, seeds=seeds[i:i + 1])
        same_jobs(alone, 0, mixed, i, f"seed {i} forward, alone")
        same_jobs(alone, 1, mixed, len(seeds) + i, f"seed {i} backward, alone")


def test_pair_switches_do_not_reach_the_tracer(backend, mixed):
    from skellysim_amd import _native
    try:
        for slices, fastpath in ((3, 1), (0, 0), (0, 2)):
            _native.set_pair_slices(slices)
            _native.set_pair_fastpath(fastpath)
            out = trace_mixed(backend)
            for j in range(len(mixed["count"])):
                same_jobs(out, j, mixed, j, f"job {j}, slices={slices} fastpath={fastpath}")
    finally:
        _native.set_pair_slices(0)
        _native.set_pair_fastpath(1)


# ---- 8. and 9. the stream contract --------------------------------------------------

def _device_sets(backend):
    import torch
    c = S.mixed_cloud()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(backend.dev)
    sets = {k: (t(v[0]), t(v[1])) for k, v in S.mixed_sets(c).items() if k != "background"}
    return sets, t(c["seeds"]), c["background"]


def test_side_stream_and_persistent_workspace(backend, mixed):
    import torch
    from skellysim_amd import _native, evaluator
    sets, seeds, background = _device_sets(backend)
    torch.cuda.synchronize()
    # The gradient pass reads the velocity functors' records, so the layout is
    # the streamline tracer's: the records of the four sets, without padding.
    needed = 8 * (9 * 301 + 12 * 97 + 6 * 5 + 9 * 3)
    lib = _native.lib()
    lib.skelly_set_persistent_ws(1)
    try:
        s = torch.cuda.Stream()
        sizes = [_block_bytes(s)]
        outs = []
        for _ in range(2):
            with torch.cuda.stream(s):
                outs.append(evaluator.trace_vortexlines_device(
                    seeds, V.ETA, **sets, background=background, dt_init=V.DT_INIT,
                    t_final=V.T_FINAL, max_points=MAX_POINTS))
            sizes.append(_block_bytes(s))
        torch.cuda.synchronize()
    finally:
        lib.skelly_set_persistent_ws(-1)
    before, first, second = sizes
    assert first >= needed and first >= before, sizes
    assert second == first, "the second call allocated again"
    for out in outs:
        host = {k: v.cpu().numpy() for k, v in out.items()}
        for j in range(len(mixed["count"])):
            same_jobs(host, j, mixed, j, f"job {j} on a side stream")


def test_streamlines_are_untouched_by_a_vortex_trace_on_their_stream(backend):
    """trace_streamlines before and after a vortex trace on one stream with the
    persistent workspace on: the vortex trace leaves nothing behind in the
    workspace the two share."""
    import torch
    from skellysim_amd import _native, evaluator
    sets, seeds, background = _device_sets(backend)
    control = dict(background=background, dt_init=S.DT_INIT, t_final=S.T_FINAL,
                   max_points=MAX_POINTS)
    lib = _native.lib()
    lib.skelly_set_persistent_ws(1)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            before = evaluator.trace_streamlines_device(seeds, S.ETA, **sets, **control)
            evaluator.trace_vortexlines_device(seeds, V.ETA, **sets, **control)
            after = evaluator.trace_streamlines_device(seeds, S.ETA, **sets, **control)
        torch.cuda.synchronize()
    finally:
        lib.skelly_set_persistent_ws(-1)
    before, after = ({k: v.cpu().numpy() for k, v in o.items()} for o in (before, after))
    assert (before["count"] > 1).all()
    for j in range(len(before["count"])):
        same_jobs(after, j, before, j, f"streamline job {j} after a vortex trace")


# ---- 10. the listener ---------------------------------------------------------------

def _vortex_request(x0, **extra):
    cmd = _request(np.zeros((0, 3)))
    cmd["vortexlines"].update(dict({"x0": np.asarray(x0, float), "t_final": 0.3}, **extra))
    return cmd


def test_listener_device_route_is_vortexlines_at_seeds(backend, trajectory):
    from skellysim_amd.flows import vortexlines_at_seeds, vorticity_from_gradient
    from skellysim_amd.listener import (Trajectory, eigen_decode, streamline_terms,
                                        velocity_gradient_field)
    sources = _sources()
    raw = _serve(trajectory, _vortex_request(X0, tracer="device"), backend, sources)
    res = msgpack.unpackb(raw[8:], raw=False)
    frame = Trajectory(trajectory).frames[0]
    want = vortexlines_at_seeds(X0, 1.0, **streamline_terms(frame, 1.0, sources=sources),
                                dt_init=0.1, t_final=0.3, backend=backend)
    assert len(res["vortexlines"]) == len(want) == len(X0) and res["streamlines"] == []
    for got, line in zip(res["vortexlines"], want):
        assert np.array_equal(eigen_decode(got["x"]), line["x"])
        assert np.array_equal(eigen_decode(got["val"]), line["val"])
        assert np.array_equal(got["time"], line["time"])
        assert got["status"] == line["status"] and len(line["x"]) >= 3
        # the field is the curl of the listener's own gradient
        w = vorticity_from_gradient(
            velocity_gradient_field(frame, line["x"], 1.0, backend, sources=sources))
        w = w.cpu().numpy() if hasattr(w, "cpu") else np.asarray(w)
        assert np.abs(line["val"] - w).max() <= 1e-10 * np.abs(w).max()


def test_listener_tracer_key_is_the_device_key_for_streamlines(backend, trajectory):
    sources = _sources()
    assert _serve(trajectory, _request(X0, tracer="device"), backend, sources) == \
        _serve(trajectory, _request(X0, device=True), backend, sources)


def test_listener_without_the_keys_never_enters_the_device_routes(backend, trajectory,
                                                                  monkeypatch):
    from skellysim_amd import flows, listener

    def never(*a, **k):
        raise AssertionError("the device route was taken")
    monkeypatch.setattr(listener, "_device_streamlines", never)
    monkeypatch.setattr(flows, "vortexlines_at_seeds", never)
    monkeypatch.setattr(flows, "streamlines_at_seeds", never)
    cmd = _request(X0[:1])
    cmd["vortexlines"].update({"x0": X0[:1], "dt_init": 0.02, "t_final": 0.05,
                               "back_integrate": False, "analytic": True})
    res = msgpack.unpackb(_serve(trajectory, cmd, backend)[8:], raw=False)
    for block in ("streamlines", "vortexlines"):
        assert len(res[block]) == 1 and "status" not in res[block][0]


# ---- 11. the C++ mirror -------------------------------------------------------------

class _VortexWithSets(_WithSets):
    def trace_vortexlines(self, seeds, eta, **kw):
        return self.backend.trace_vortexlines(seeds, eta, **dict(kw, **self.sets))


def test_cpp_mirror_prints_the_python_line(backend, tmp_path):
    """tests/fieldline_probe.cpp (vortexlines) through include/skelly_evaluator.hpp
    (the host form) against flows.vortexlines_at_seeds (the device form), all four
    sets, the background and a body: the same joined line, bit for bit."""
    from skellysim_amd.flows import vortexlines_at_seeds
    c = S.mixed_cloud()
    body = np.array([[0.0, 0.0, 0.0, 0.05, 0.1, 0.0, 0.0, 0.0, 0.0, 1.0]])
    cxx = next((x for x in (os.environ.get("CXX"), "g++", "c++", "clang++")
                if x and shutil.which(x)), None)
    assert cxx, "no host C++ compiler"
    exe, case = str(tmp_path / "fieldline_probe"), str(tmp_path / "case.bin")
    libdir = os.path.join(REPO, "skellysim_amd")
    built = subprocess.run(
        [cxx, "-O2", "-std=c++17", "-I", os.path.join(REPO, "include"),
         os.path.join(REPO, "tests", "fieldline_probe.cpp"), "-L", libdir, "-lskellyhip",
         "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    order = ("stokeslet", "stresslet", "rotlet", "oseen")
    uniform, scale, comp = c["background"]
    with open(case, "wb") as f:
        np.array([len(c[k][0]) for k in order] + [len(body), len(c["seeds"]), 1, MAX_POINTS, 1],
                 np.int64).tofile(f)
        np.array([V.ETA, 5e-3, 1e-5, V.DT_INIT, V.T_FINAL, 1e-10, 1e-6, *uniform, *scale, *comp],
                 np.float64).tofile(f)
        for k in order:
            for a in c[k]:
                np.ascontiguousarray(a, np.float64).tofile(f)
        body.tofile(f)
        np.ascontiguousarray(c["seeds"]).tofile(f)
    seed = 3
    r = subprocess.run([exe, "vortexlines", case, str(seed)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, f"fieldline_probe failed ({r.returncode}): {r.stdout} {r.stderr}"
    head, *rows = r.stdout.strip().splitlines()
    got = np.array([[float(v) for v in row.split()] for row in rows])

    to = lambda a: np.ascontiguousarray(a, np.float64)
    line = vortexlines_at_seeds(
        c["seeds"], V.ETA,
        fiber=dict(r_src=to(c["stokeslet"][0]), forces=to(c["stokeslet"][1]),
                   weights=np.ones(len(c["stokeslet"][0]))),
        sources=dict(force_pos=c["oseen"][0], forces=c["oseen"][1], torque_pos=c["rotlet"][0],
                     torques=c["rotlet"][1], background=c["background"]),
        max_points=MAX_POINTS,
        backend=_VortexWithSets(backend, stresslet=c["stresslet"], bodies=body),
    )[seed]
    assert head == f"lines {len(c['seeds'])} status {line['status']} points {len(line['x'])}"
    assert np.array_equal(got[:, 0], line["time"])
    assert np.array_equal(got[:, 1:4], line["x"]) and np.array_equal(got[:, 4:7], line["val"])
