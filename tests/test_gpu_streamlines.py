"""The device streamline tracer against the CPU reference of
tests/streamline_reference.py, and the layers above it.

The comparison with the reference is on the mixed cloud of that file (301
Stokeslets: one full pass of a 256-thread workgroup and a remainder; 97
stresslets, 5 rotlets and 3 regularized Stokeslets: less than one pass; the
background on), 7 seeds both ways. Points are not compared one by one: a
rounding-size change of the velocity moves the step sizes, hence the times
of the intermediate points (tests/test_streamlines_cpu.py, precondition (b)).
What is compared is what that precondition shows to be stable, two decades
under the bounds used here: count, status, end point and times. Every
recorded step is then replayed on its own with oracle velocities, which holds
each intermediate point to the stepper."""

import ctypes
import io
import os
import shutil
import struct
import subprocess

import msgpack
import numpy as np
import pytest

import streamline_reference as S

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS = 128  # the longest reference run of the mixed cloud has 43 points


@pytest.fixture(scope="module")
def backend(hip_lib_path):
    from skellysim_amd.system_fd import HipBackend
    return HipBackend()


def trace_mixed(backend, seeds=None, **kw):
    c = S.mixed_cloud()
    kw = dict(dict(dt_init=S.DT_INIT, t_final=S.T_FINAL, back_integrate=True,
                   max_points=MAX_POINTS), **kw)
    return backend.trace_streamlines(c["seeds"] if seeds is None else seeds, S.ETA,
                                     **S.mixed_sets(c), **kw)


@pytest.fixture(scope="module")
def mixed(backend):
    return trace_mixed(backend)


def job_rows(out, j):
    """What job j wrote: (x, t, val, count, status)."""
    c = int(out["count"][j])
    return out["x"][j, :c], out["t"][j, :c], out["val"][j, :c], c, int(out["status"][j])


def same_jobs(a, ja, b, jb, what):
    ra, rb = job_rows(a, ja), job_rows(b, jb)
    assert ra[3:] == rb[3:], f"{what}: count/status {ra[3:]} against {rb[3:]}"
    for u, v, name in zip(ra[:3], rb[:3], ("x", "t", "val")):
        assert np.array_equal(u, v), f"{what}: {name} differs"


# ---- 1. the mixed cloud against the reference ---------------------------------------

def test_mixed_cloud_matches_the_reference(oracle_mod, mixed):
    c = S.mixed_cloud()
    pts = np.concatenate([c[k][0] for k in ("stokeslet", "stresslet", "rotlet", "oseen")]
                         + [c["seeds"]])
    extent = float(np.max(pts.max(axis=0) - pts.min(axis=0)))
    assert (mixed["count"] >= 0).all(), "a job never ran"
    kept = S.kept_seeds()
    assert len(kept) >= 5
    for j, (i, tf, ref) in enumerate(S.mixed_reference()):
        if i not in kept:
            continue
        x, t, val, count, status = job_rows(mixed, j)
        end = np.abs(x[-1] - ref["x"][-1]).max() if count == ref["count"] else np.nan
        times = np.abs(t - ref["t"]).max() if count == ref["count"] else np.nan
        print(f"seed {i} t_final {tf:+.0f}: count {count} ({ref['count']}), status {status} "
              f"({ref['status']}), end {end:.2e}, times {times:.2e}")
        assert (status, count) == (ref["status"], ref["count"]), (i, tf)
        assert end <= 1e-10 * extent, (i, tf, end)
        assert times <= 1e-6, (i, tf, times)
        assert t[0] == 0.0 and np.array_equal(x[0], c["seeds"][i])
        if status == S.DONE:
            assert abs(t[-1] - tf) <= S.EPS  # the loop's own exit condition


def test_mixed_cloud_val_is_the_oracle_velocity(oracle_mod, mixed):
    f = S.cloud_field(oracle_mod, S.ETA, **S.mixed_sets())
    worst = 0.0
    for j in range(len(mixed["count"])):
        x, _, val, _, _ = job_rows(mixed, j)
        u = f(x)
        rel = np.linalg.norm(val - u, axis=1) / np.linalg.norm(u, axis=1)
        worst = max(worst, rel.max())
        assert rel.max() <= 1e-10, (j, rel.max())
    print(f"val against the oracle: {worst:.2e} relative")


def test_mixed_cloud_steps_replay(oracle_mod, mixed):
    """From each recorded (x_k, t_{k+1} - t_k) one Cash-Karp step with oracle
    velocities lands on x_{k+1} within 1e-10 |dt| max|k_i| plus 4 ulp of |x|,
    and has err <= 1 (it was an accepted step)."""
    f = S.cloud_field(oracle_mod, S.ETA, **S.mixed_sets())
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


# ---- 2. rigid rotation --------------------------------------------------------------

W = 2.0
SEED = np.array([[0.7, -0.2, 0.3]])


def _rotated(p, angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c * p[0] - s * p[1], s * p[0] + c * p[1], p[2]])


@pytest.mark.parametrize("how", ["background", "body"])
def test_rigid_rotation(backend, oracle_mod, how):
    """u = w e_z x x once as the background term and once as the motion of a
    body that holds the seed: the end point is as close to the analytic one as
    the CPU reference's, to 1e-10."""
    if how == "background":
        field = dict(background=((0.0, 0.0, 0.0), (-W, W, 0.0), (1, 0, 2)))
    else:
        # both bodies hold the whole path: the later one decides
        field = dict(bodies=np.array([[0.0, 0.0, 0.0, 5.0, 3.0, 3.0, 3.0, 1.0, 1.0, 1.0],
                                      [0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, W]]))
    out = backend.trace_streamlines(SEED, 1.0, **field, max_points=MAX_POINTS)
    f = S.cloud_field(oracle_mod, 1.0, **field)
    for j, tf in enumerate((1.0, -1.0)):
        ref = S.trace(f, SEED[0], 0.1, tf)
        x, t, val, count, status = job_rows(out, j)
        exact = _rotated(SEED[0], W * tf)
        mine, theirs = np.linalg.norm(x[-1] - exact), np.linalg.norm(ref["x"][-1] - exact)
        print(f"{how} t_final {tf:+.0f}: {count} points, {mine:.2e} from the analytic end "
              f"(reference {theirs:.2e})")
        assert (status, count) == (S.DONE, ref["count"]) and abs(t[-1] - tf) <= S.EPS
        assert mine <= theirs + 1e-10
        assert np.abs(val - f(x)).max() <= 1e-14 * W


# ---- 3. statuses --------------------------------------------------------------------

def test_strong_stokeslet_is_a_singularity(backend, oracle_mod):
    sl = (np.array([[0.0, 0.0, 0.0]]), np.array([[1e6, 0.0, 0.0]]))
    seed = np.array([[0.1, 0.05, 0.0]])
    out = backend.trace_streamlines(seed, 1.0, stokeslet=sl, max_points=MAX_POINTS)
    u = oracle_mod.stokeslet(sl[0], sl[1], seed, 1.0)
    assert np.linalg.norm(u) > 1e3
    for j in range(2):
        x, t, val, count, status = job_rows(out, j)
        assert (status, count) == (S.SINGULAR, 1)
        assert np.array_equal(x, seed) and t[0] == 0.0
        assert np.abs(val - u).max() <= 1e-10 * np.abs(u).max()


def test_full_buffer(backend, mixed):
    out = trace_mixed(backend, max_points=4)
    long_jobs = [j for j in range(len(mixed["count"])) if mixed["count"][j] > 4]
    assert long_jobs
    for j in range(len(mixed["count"])):
        if j in long_jobs:
            assert (int(out["count"][j]), int(out["status"][j])) == (4, S.FULL)
            assert np.array_equal(out["x"][j], mixed["x"][j, :4])
            assert np.array_equal(out["t"][j], mixed["t"][j, :4])
        else:
            same_jobs(out, j, mixed, j, f"job {j} that fits 4 points")


def test_empty_sets(backend, oracle_mod):
    """Stokeslets and rotlets alone (no stresslet, no oseen, no background), at
    eta = 1: against the reference as the mixed cloud is."""
    c = S.mixed_cloud()
    sets = dict(stokeslet=c["stokeslet"], rotlet=c["rotlet"])
    seeds = c["seeds"][:2]
    out = backend.trace_streamlines(seeds, 1.0, **sets, stresslet=None,
                                    oseen=(np.zeros((0, 3)), np.zeros((0, 3))),
                                    max_points=MAX_POINTS)
    f = S.cloud_field(oracle_mod, 1.0, **sets)
    for j, (i, tf) in enumerate([(0, 1.0), (1, 1.0), (0, -1.0), (1, -1.0)]):
        ref = S.trace(f, seeds[i], 0.1, tf)
        x, t, val, count, status = job_rows(out, j)
        assert (status, count) == (ref["status"], ref["count"]), (i, tf)
        assert np.abs(x[-1] - ref["x"][-1]).max() <= 2e-10
        assert np.abs(t - ref["t"]).max() <= 1e-6


def test_no_sources_at_all(backend):
    out = backend.trace_streamlines(SEED, 1.0, background=((0.5, 0.0, 0.0), (0, 0, 0), (0, 1, 2)),
                                    back_integrate=False, max_points=MAX_POINTS)
    x, t, val, count, status = job_rows(out, 0)
    assert status == S.DONE and abs(t[-1] - 1.0) <= S.EPS
    assert np.abs(x[-1] - (SEED[0] + [0.5, 0.0, 0.0])).max() <= 1e-14


def test_zero_seeds(backend):
    from skellysim_amd.flows import streamlines_at_seeds
    out = backend.trace_streamlines(np.zeros((0, 3)), 1.0, **S.mixed_sets())
    assert out["count"].shape == (0,) and out["x"].shape[0] == 0
    assert streamlines_at_seeds(np.zeros((0, 3)), 1.0, backend=backend) == []


# ---- 4. determinism -----------------------------------------------------------------

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


# ---- 5. the stream contract ---------------------------------------------------------

def _block_bytes(stream):
    from skellysim_amd import _native
    n = ctypes.c_longlong(-1)
    assert _native.lib().skelly_persistent_ws_bytes(ctypes.c_void_p(stream.cuda_stream),
                                                    ctypes.byref(n)) == 0
    return n.value


def test_side_stream_and_persistent_workspace(backend, mixed):
    import torch
    from skellysim_amd import _native, evaluator
    c = S.mixed_cloud()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(backend.dev)
    sets = {k: (t(v[0]), t(v[1])) for k, v in S.mixed_sets(c).items() if k != "background"}
    seeds = t(c["seeds"])
    torch.cuda.synchronize()
    # the records of the four sets, without their padding
    needed = 8 * (9 * 301 + 12 * 97 + 6 * 5 + 9 * 3)
    lib = _native.lib()
    lib.skelly_set_persistent_ws(1)
    try:
        s = torch.cuda.Stream()
        sizes = [_block_bytes(s)]
        outs = []
        for _ in range(2):
            with torch.cuda.stream(s):
                outs.append(evaluator.trace_streamlines_device(
                    seeds, S.ETA, **sets, background=c["background"], dt_init=S.DT_INIT,
                    t_final=S.T_FINAL, max_points=MAX_POINTS))
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


# ---- 6. the listener ----------------------------------------------------------------

@pytest.fixture(scope="module")
def trajectory(tmp_path_factory, backend):
    from skellysim_amd.fiber_fd import FiberFD
    from skellysim_amd.system_fd import SystemFD
    from skellysim_amd.trajectory import TrajectoryWriter
    s = np.linspace(0, 1.0, 24)
    x = np.stack([0.15 * np.sin(2 * np.pi * s), np.zeros_like(s), s], axis=1)
    fib = FiberFD(x, length=1.0, bending_rigidity=2.5e-2, eta=1.0)
    sys_ = SystemFD([fib], eta=1.0, dt=0.1, backend=backend)
    path = str(tmp_path_factory.mktemp("streamlines") / "skelly_sim.out")
    with TrajectoryWriter(path) as tw:
        tw.write_frame(sys_, 0.1, 0.1)
    return path


def _serve(path, cmd, compute, sources=None):
    from skellysim_amd.listener import Trajectory, serve
    from test_listener import _ndencode
    msg = msgpack.packb(cmd, default=_ndencode)
    stdin = io.BytesIO(struct.pack("<Q", len(msg)) + msg + struct.pack("<Q", 0))
    stdout = io.BytesIO()
    serve(stdin, stdout, Trajectory(path), compute, eta=1.0, sources=sources)
    raw = stdout.getvalue()
    (size,) = struct.unpack("<Q", raw[:8])
    assert len(raw) == 8 + size
    return raw


def _request(x0, **extra):
    return {
        "frame_no": 0, "evaluator": "GPU",
        "streamlines": dict({"dt_init": 0.1, "t_final": 0.3, "abs_err": 1e-10, "rel_err": 1e-6,
                             "back_integrate": True, "x0": np.asarray(x0, float)}, **extra),
        "vortexlines": {"dt_init": 0.1, "t_final": 1.0, "abs_err": 1e-10, "rel_err": 1e-6,
                        "back_integrate": True, "x0": np.zeros((0, 3))},
        "velocity_field": {"x": np.zeros((0, 3))},
    }


X0 = np.array([[0.6, 0.2, 0.4], [-0.3, 0.4, 0.8]])


def _sources():
    from skellysim_amd.sources import BackgroundSource, PointSource, PointSourceContainer
    psc = PointSourceContainer([PointSource((0.9, 0.9, 0.1), force=(0.5, 0.0, -0.2)),
                                PointSource((-0.8, 0.1, 0.2), torque=(0.0, 0.3, 0.1)),
                                PointSource((0.0, 0.9, 0.9), force=(9.0, 9.0, 9.0),
                                            time_to_live=0.05)])  # dead at the frame's 0.1
    return psc, BackgroundSource((1, 2, 0), (0.3, -0.2, 0.1), (0.05, 0.0, -0.05))


def test_listener_device_route_is_streamlines_at_seeds(backend, trajectory):
    from skellysim_amd.flows import streamlines_at_seeds
    from skellysim_amd.listener import Trajectory, eigen_decode, streamline_terms, velocity_field
    sources = _sources()
    raw = _serve(trajectory, _request(X0, device=True), backend, sources)
    res = msgpack.unpackb(raw[8:], raw=False)
    frame = Trajectory(trajectory).frames[0]
    want = streamlines_at_seeds(X0, 1.0, **streamline_terms(frame, 1.0, sources=sources),
                                dt_init=0.1, t_final=0.3, backend=backend)
    assert len(res["streamlines"]) == len(want) == len(X0)
    for got, line in zip(res["streamlines"], want):
        assert np.array_equal(eigen_decode(got["x"]), line["x"])
        assert np.array_equal(eigen_decode(got["val"]), line["val"])
        assert np.array_equal(got["time"], line["time"])
        assert got["status"] == line["status"] == S.DONE
        assert abs(line["time"][0] + 0.3) <= S.EPS and abs(line["time"][-1] - 0.3) <= S.EPS
        # the field is the listener's own
        u = velocity_field(frame, line["x"], 1.0, backend, sources=sources)
        assert np.abs(line["val"] - u).max() <= 1e-10 * np.abs(u).max()


def test_listener_without_the_key_takes_the_host_route(backend, trajectory, monkeypatch):
    """No key, or a false one: the bytes of the host route (scipy's RK45 over
    velocity_field, as before the device route existed), which is never
    entered."""
    from skellysim_amd import listener
    from skellysim_amd.listener import (Trajectory, eigen_encode_3xn, integrate_streamline,
                                        velocity_field)

    def never(*a, **k):
        raise AssertionError("the device route was taken")
    monkeypatch.setattr(listener, "_device_streamlines", never)
    plain = _serve(trajectory, _request(X0[:1]), backend)
    keyed = msgpack.unpackb(_serve(trajectory, _request(X0[:1], device=False), backend)[8:])
    res = msgpack.unpackb(plain[8:], raw=False)
    assert keyed == res
    frame = Trajectory(trajectory).frames[0]
    s = integrate_streamline(lambda p: velocity_field(frame, p, 1.0, backend), X0[0],
                             dt_init=0.1, t_final=0.3)
    assert res["streamlines"] == [{"x": eigen_encode_3xn(s["x"]), "val": eigen_encode_3xn(s["val"]),
                                   "time": s["time"]}]


def test_vortex_lines_ignore_the_key(backend, trajectory, monkeypatch):
    from skellysim_amd import listener

    def never(*a, **k):
        raise AssertionError("the device route was taken")
    monkeypatch.setattr(listener, "_device_streamlines", never)
    cmd = _request(np.zeros((0, 3)))
    cmd["vortexlines"].update({"x0": X0[:1], "dt_init": 0.02, "t_final": 0.05, "device": True,
                               "back_integrate": False, "analytic": True})
    res = msgpack.unpackb(_serve(trajectory, cmd, backend)[8:], raw=False)
    assert len(res["vortexlines"]) == 1 and "status" not in res["vortexlines"][0]


# ---- 7. the C++ mirror --------------------------------------------------------------

def test_cpp_mirror_prints_the_python_line(backend, tmp_path):
    """tests/fieldline_probe.cpp (streamlines) through include/skelly_evaluator.hpp
    (the host form) against flows.streamlines_at_seeds (the device form), all four
    sets, the background and a body: the same joined line, bit for bit."""
    from skellysim_amd.flows import streamlines_at_seeds
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
        np.array([S.ETA, 5e-3, 1e-5, S.DT_INIT, S.T_FINAL, 1e-10, 1e-6, *uniform, *scale, *comp],
                 np.float64).tofile(f)
        for k in order:
            for a in c[k]:
                np.ascontiguousarray(a, np.float64).tofile(f)
        body.tofile(f)
        np.ascontiguousarray(c["seeds"]).tofile(f)
    seed = 3
    r = subprocess.run([exe, "streamlines", case, str(seed)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, f"fieldline_probe failed ({r.returncode}): {r.stdout} {r.stderr}"
    head, *rows = r.stdout.strip().splitlines()
    got = np.array([[float(v) for v in row.split()] for row in rows])

    to = lambda a: np.ascontiguousarray(a, np.float64)
    line = streamlines_at_seeds(
        c["seeds"], S.ETA,
        fiber=dict(r_src=to(c["stokeslet"][0]), forces=to(c["stokeslet"][1]),
                   weights=np.ones(len(c["stokeslet"][0]))),
        sources=dict(force_pos=c["oseen"][0], forces=c["oseen"][1], torque_pos=c["rotlet"][0],
                     torques=c["rotlet"][1], background=c["background"]),
        max_points=MAX_POINTS, backend=_WithSets(backend, stresslet=c["stresslet"], bodies=body),
    )[seed]
    assert head == f"lines {len(c['seeds'])} status {line['status']} points {len(line['x'])}"
    assert np.array_equal(got[:, 0], line["time"])
    assert np.array_equal(got[:, 1:4], line["x"]) and np.array_equal(got[:, 4:7], line["val"])


class _WithSets:
    """A backend that adds a raw stresslet set and raw body rows to what
    streamlines_at_seeds assembles (its own terms build them from normals and
    densities, which the cloud does not have)."""

    def __init__(self, backend, **sets):
        self.backend, self.sets, self.dev = backend, sets, backend.dev

    def _t(self, a):
        return self.backend._t(a)

    def trace_streamlines(self, seeds, eta, **kw):
        return self.backend.trace_streamlines(seeds, eta, **dict(kw, **self.sets))
