"""GPU tests of the pressure kernels (csrc/pair_functors.hpp: StokesletPressure,
which is also the regularized Oseen pressure, and StressletPressure, through
the shared pair driver) and of the stress layers on top of them.

Per target, every result is held to

    |out - ref| <= bound(A, n_src, n_slices, kernel)

against the longdouble references of tests/pressure_reference.py (A the
condition sum; an entry with A == 0 has to be exactly 0), over every case of
tests/pair_cases.py at its forced slice counts, as test_gpu_pair_accuracy.py
does for the velocity and gradient functors. MAX_TPT of both functors is 4, the
velocity functors' own, so CASES' 1, 513 and 1025 targets reach every
targets-a-thread build and no further cloud is needed for a partially filled
thread. The compositions (flows, listener, surface integrals) are compared
with the numpy backend of tests/test_pressure_cpu.py."""

import ctypes
import os
import shutil
import struct
import subprocess
from dataclasses import replace

import msgpack
import numpy as np
import pytest

import pair_cases as PC
import pressure_reference as PR
from test_gpu_pair_accuracy import judge
from test_gpu_pair_slices import sliced
from test_pressure_cpu import NumpyPressureBackend, cloud37, sphere_quadrature
from test_gradient_cpu import far_probes, rel, _ndencode

pytestmark = pytest.mark.gpu

ETA = 1.3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


# host forms and device forms by pressure_reference.KERNELS name
EVALUATE = {
    "stokeslet_pressure": lambda ska, c: ska.stokeslet_pressure(c.r_src, c.f3, c.r_trg),
    "stresslet_pressure": lambda ska, c: ska.stresslet_pressure(c.r_src, c.f9, c.r_trg),
    "oseen_pressure": lambda ska, c: ska.oseen_contract_pressure(c.r_src, c.r_trg, c.f3, c.reg,
                                                                 c.eps),
}
DEVICE = {
    "stokeslet_pressure": lambda ska, c, out=None: ska.stokeslet_pressure_device(
        _t(c.r_src), _t(c.f3), _t(c.r_trg), out=out),
    "stresslet_pressure": lambda ska, c, out=None: ska.stresslet_pressure_device(
        _t(c.r_src), _t(c.f9), _t(c.r_trg), out=out),
    "oseen_pressure": lambda ska, c, out=None: ska.oseen_contract_pressure_device(
        _t(c.r_src), _t(c.r_trg), _t(c.f3), c.reg, c.eps, out=out),
}
assert list(EVALUATE) == PR.KERNELS


def fetch(fn, stream=None):
    import torch
    if stream is None:
        out = fn()
    else:
        with torch.cuda.stream(stream):
            out = fn()
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- per-target bound -------------------------------------------------------

def run_case(ska, kernel, name, case, n_slices):
    ref, A = PR.reference(name, kernel, case)
    p_on, p_again, p_off = sliced(n_slices, lambda: EVALUATE[kernel](ska, case))
    assert p_on.shape == (len(case.r_trg),)
    assert np.array_equal(p_on, p_again, equal_nan=True), "two consecutive calls differ"
    assert np.array_equal(p_on, p_off, equal_nan=True), "the fast-path switch changed the result"
    limit = PR.bound(A, case.n_src, min(n_slices, case.n_src), kernel)
    judge(f"{kernel} {name} slices={n_slices}", p_on, ref, A, limit)


def _runs(cases, kernels):
    return [(k, n, s) for n, (_, slices) in cases.items() for s in slices for k in kernels]


@pytest.mark.parametrize("kernel,name,n_slices", _runs(PC.CASES, PR.KERNELS))
def test_pressure_within_bound(ska, kernel, name, n_slices):
    run_case(ska, kernel, name, PC.CASES[name][0], n_slices)


@pytest.mark.parametrize("kernel,name,n_slices", _runs(PC.THRESHOLD_CASES, ["oseen_pressure"]))
def test_oseen_pressure_threshold_within_bound(ska, kernel, name, n_slices):
    """Pairs just either side of the `r2 > eps^2` comparison, and the near
    cloud with other reg and eps."""
    run_case(ska, kernel, name, PC.THRESHOLD_CASES[name][0], n_slices)


@pytest.mark.parametrize("kernel,name,n_slices", _runs(PC.REG0_CASES, ["oseen_pressure"]))
def test_oseen_pressure_reg_zero_on_coincident_points(ska, kernel, name, n_slices):
    """reg = 0: a coincident pair has den = 0 and only the mask keeps it out."""
    run_case(ska, kernel, name, PC.REG0_CASES[name][0], n_slices)


@pytest.mark.parametrize("kernel", PR.KERNELS)
def test_self_cloud_is_finite(ska, kernel):
    """Every target on a source, three points duplicated: no NaN, no inf, and
    inside the bound (default reg)."""
    case = PC.self_cloud()
    out = EVALUATE[kernel](ska, case)
    assert np.isfinite(out).all()
    ref, A = PR.reference("self_default", kernel, case)
    judge(f"{kernel} self_cloud", out, ref, A, PR.bound(A, case.n_src, 1, kernel))


# ---- fast path and determinism ------------------------------------------------

@pytest.mark.parametrize("kernel", PR.KERNELS)
def test_fastpath_modes_and_repeat_are_bitwise_equal(ska, kernel):
    """One launch of 8192 sources x 257 targets, where the auto mode switches
    the fast path on for the functors that have one, 3 of the targets placed on
    sources: bitwise equal under skelly_set_pair_fastpath 0, 1 and 2 and on a
    repeat, finite, and inside the bound."""
    from skellysim_amd import _native
    case = PC.cloud(8192, 8192, 257)
    case.r_trg[[5, 100, 256]] = case.r_src[[0, 4097, 8191]]
    d = {k: _t(getattr(case, k)) for k in ("r_src", "r_trg", "f3", "f9")}
    call = {
        "stokeslet_pressure": lambda: ska.stokeslet_pressure_device(d["r_src"], d["f3"],
                                                                    d["r_trg"]),
        "stresslet_pressure": lambda: ska.stresslet_pressure_device(d["r_src"], d["f9"],
                                                                    d["r_trg"]),
        "oseen_pressure": lambda: ska.oseen_contract_pressure_device(d["r_src"], d["r_trg"],
                                                                     d["f3"]),
    }[kernel]
    try:
        _native.set_pair_slices(1)
        got = {}
        for mode in (0, 1, 2):
            _native.set_pair_fastpath(mode)
            got[mode] = fetch(call)
        _native.set_pair_fastpath(1)
        again = fetch(call)
    finally:
        _native.set_pair_fastpath(1)
        _native.set_pair_slices(0)
    assert np.isfinite(got[1]).all()
    for mode in (0, 2):
        assert np.array_equal(got[mode], got[1]), f"fastpath {mode} differs from auto"
    assert np.array_equal(again, got[1]), "a repeat differs"
    ref, A = PR.reference("fastpath_8192x257", kernel, case)
    judge(f"{kernel} 8192x257", got[1], ref, A, PR.bound(A, case.n_src, 1, kernel))


# ---- forms agree ----------------------------------------------------------------

@pytest.mark.parametrize("kernel", PR.KERNELS)
def test_host_and_device_forms_agree(ska, kernel):
    case = PC.CASES["driver_131x513"][0]
    dev = fetch(lambda: DEVICE[kernel](ska, case))
    assert dev.shape == (513,)
    assert np.array_equal(dev, EVALUATE[kernel](ska, case))


# ---- the device forms' contract ---------------------------------------------------

@pytest.mark.parametrize("kernel", PR.KERNELS)
def test_device_form_on_a_side_stream_and_into_out(ska, kernel):
    import torch
    case = PC.CASES["driver_131x513"][0]
    want = EVALUATE[kernel](ska, case)
    side = torch.cuda.Stream()
    assert np.array_equal(fetch(lambda: DEVICE[kernel](ska, case), side), want)
    out = torch.full((513,), float("nan"), dtype=torch.float64, device="cuda:0")
    with torch.cuda.stream(side):
        assert DEVICE[kernel](ska, case, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    for bad in (torch.zeros(512, dtype=torch.float64, device="cuda:0"),
                torch.zeros(513, dtype=torch.float32, device="cuda:0"), np.zeros(513)):
        with pytest.raises(ValueError, match="out"):
            DEVICE[kernel](ska, case, out=bad)


@pytest.mark.parametrize("kernel", PR.KERNELS)
def test_device_form_zero_sources_and_zero_targets(ska, kernel):
    import torch
    case = PC.CASES["driver_131x513"][0]
    none = replace(case, r_src=np.zeros((0, 3)), f3=np.zeros((0, 3)), f9=np.zeros((0, 9)))
    out = torch.full((513,), float("nan"), dtype=torch.float64, device="cuda:0")
    DEVICE[kernel](ska, none, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0).all()
    empty = fetch(lambda: DEVICE[kernel](ska, replace(case, r_trg=np.zeros((0, 3)))))
    assert empty.shape == (0,)


@pytest.mark.parametrize("name", ["skelly_stokeslet_pressure_device",
                                  "skelly_stresslet_pressure_device",
                                  "skelly_oseen_contract_pressure_device"])
@pytest.mark.parametrize("bad", [0, 1], ids=["n_src", "n_trg"])
def test_device_form_negative_count(ska, name, bad):
    """Real device pointers and a negative count: the negative-size error with
    its message, and the output as it was."""
    import threading
    import torch
    from skellysim_amd import _native
    lib = _native.lib()
    case = PC.CASES["driver_131x513"][0]
    r_src, r_trg = _t(case.r_src), _t(case.r_trg)
    f = _t(case.f9 if "stresslet" in name else case.f3)
    out = torch.full((513,), -12345.678, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    counts = [131, 513]
    counts[bad] = -1
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if "oseen" in name:
        args = (p(r_src), p(r_trg), p(f), p(out), counts[0], counts[1], 5e-3, 1e-5, stream)
    else:
        args = (p(r_src), p(f), counts[0], p(r_trg), p(out), counts[1], stream)
    got = []

    def run():  # the message is per thread
        got.append(getattr(lib, name)(*args))
        got.append(lib.skelly_hip_last_error().decode())
    t = threading.Thread(target=run)
    t.start()
    t.join()
    torch.cuda.synchronize()
    assert got[0] != 0 and got[1] == name + ": negative size", got
    assert (out.cpu().numpy() == -12345.678).all()


# ---- composition on the device -------------------------------------------------------

def _composition_inputs(golden_dir):
    """Fiber + shell + body inputs: the committed periphery sphere as the
    shell, the committed body sphere at radius 0.3 with two centers."""
    rng = np.random.default_rng(8)
    sh = np.load(os.path.join(golden_dir, "periphery_sphere_192.npz"))
    bd = np.load(os.path.join(golden_dir, "body_sphere_600.npz"))
    body_normals = np.asarray(bd["normals"], float)
    body_nodes = 0.3 * body_normals / np.linalg.norm(body_normals, axis=1)[:, None]
    fib = dict(r_src=rng.uniform(-0.5, 0.5, (70, 3)), forces=rng.uniform(-1, 1, (70, 3)),
               weights=rng.uniform(0.1, 0.2, 70))
    shell = dict(node_pos=np.asarray(sh["nodes"], float), node_normal=np.asarray(sh["normals"],
                                                                              float),
                 density=rng.uniform(-1, 1, (len(sh["nodes"]), 3)))
    bodies = dict(node_pos=body_nodes, node_normals=body_normals,
                  densities=rng.uniform(-1, 1, (len(body_nodes), 3)),
                  centers=rng.uniform(-0.2, 0.2, (2, 3)), forces=rng.uniform(-1, 1, (2, 3)),
                  torques=rng.uniform(-1, 1, (2, 3)))
    pts = np.concatenate([fib["r_src"], shell["node_pos"], body_nodes])
    r_trg = far_probes(pts, 33, seed=14, box=0.9 * float(np.linalg.norm(shell["node_pos"],
                                                                        axis=1).min()),
                       clearance=0.15)
    return fib, shell, bodies, r_trg


def test_flows_pressure_and_stress_composition(ska, golden_dir):
    """flows.pressure_at_targets and stress_at_targets on device tensors
    (HipBackend by default) against the numpy backend, 1e-12 norm-relative."""
    import torch
    from skellysim_amd.flows import pressure_at_targets, stress_at_targets
    fib, shell, bodies, r_trg = _composition_inputs(golden_dir)
    dev = lambda d: {k: _t(v) for k, v in d.items()}
    p = pressure_at_targets(_t(r_trg), ETA, fiber=dev(fib), shell=dev(shell), bodies=dev(bodies))
    sigma = stress_at_targets(_t(r_trg), ETA, fiber=dev(fib), shell=dev(shell),
                              bodies=dev(bodies))
    torch.cuda.synchronize()
    assert torch.is_tensor(p) and p.shape == (33,) and sigma.shape == (33, 3, 3)
    be = NumpyPressureBackend()
    p_ref = pressure_at_targets(r_trg, ETA, fiber=fib, shell=shell, bodies=bodies, backend=be)
    s_ref = stress_at_targets(r_trg, ETA, fiber=fib, shell=shell, bodies=bodies, backend=be)
    print("composition: pressure", rel(p.cpu().numpy(), p_ref), "stress",
          rel(sigma.cpu().numpy(), s_ref))
    assert np.linalg.norm(p_ref) > 0
    assert rel(p.cpu().numpy(), p_ref) < 1e-12
    assert rel(sigma.cpu().numpy(), s_ref) < 1e-12


def test_traction_integrals_on_the_device(ska):
    """The 2048-point sphere of radius 3 around 37 sources, through HipBackend:
    Stokeslets carry F = -sum f, T = -sum s x f; stresslets nothing; rotlets
    T = -sum torque. 1e-12 absolute."""
    from skellysim_amd.flows import stress_at_targets, surface_force_torque
    from skellysim_amd.system_fd import HipBackend
    src, f3, _, torque = cloud37()
    pts, nrm, w = sphere_quadrature()
    assert len(pts) == 2048
    be = HipBackend()
    z = np.zeros((0, 3))
    cases = {
        "stokeslets": (dict(fiber=dict(r_src=src, forces=f3, weights=np.ones(len(src)))),
                       -f3.sum(axis=0), -np.cross(src, f3).sum(axis=0)),
        "stresslets": (dict(shell=dict(node_pos=src, node_normal=f3, density=torque)),
                       np.zeros(3), np.zeros(3)),
        "rotlets": (dict(bodies=dict(node_pos=z, node_normals=z, densities=z, centers=src,
                                     forces=np.zeros_like(src), torques=torque)),
                    np.zeros(3), -torque.sum(axis=0)),
    }
    worst = {}
    for name, (terms, F_want, T_want) in cases.items():
        sigma = stress_at_targets(pts, ETA, backend=be, **terms)
        assert isinstance(sigma, np.ndarray)
        F, T = surface_force_torque(pts, nrm, w, sigma, np.zeros(3))
        worst[name] = (np.abs(F - F_want).max(), np.abs(T - T_want).max())
        print("traction integrals", name, worst[name])
    for name, (dF, dT) in worst.items():
        assert dF < 1e-12 and dT < 1e-12, (name, dF, dT)


# ---- listener over HIP -----------------------------------------------------------------

def test_listener_pressure_and_stress_hip(tmp_path, hip_lib_path):
    """One "pressure" + "stress" request served by HipBackend against the
    numpy backend's answer for the same frame, at the norm-relative parity bar
    of the other listener tests on the device (1e-10)."""
    from skellysim_amd.fiber_fd import FiberFD
    from skellysim_amd.system_fd import SystemFD, HipBackend
    from skellysim_amd.trajectory import TrajectoryWriter
    from skellysim_amd.listener import Trajectory, eigen_decode, pressure_field, stress_field
    from test_listener import _roundtrip

    s = np.linspace(0, 1.0, 24)
    x = np.stack([0.15 * np.sin(2 * np.pi * s), np.zeros_like(s), s], axis=1)
    fib = FiberFD(x, length=1.0, bending_rigidity=2.5e-2, eta=1.0)
    compute = HipBackend()
    sys_ = SystemFD([fib], eta=1.0, dt=0.1, backend=compute)
    path = str(tmp_path / "skelly_sim.out")
    with TrajectoryWriter(path) as tw:
        tw.write_frame(sys_, 0.1, 0.1)
    frame = Trajectory(path).frames[0]
    probes = far_probes(x, 16, seed=6)
    cmd = {
        "frame_no": 0,
        "evaluator": "GPU",
        "streamlines": {"x0": np.zeros((0, 3))},
        "vortexlines": {"x0": np.zeros((0, 3))},
        "velocity_field": {"x": np.zeros((0, 3))},
        "pressure": {"x": probes},
        "stress": {"x": probes},
    }
    msg = msgpack.packb(cmd, default=_ndencode)
    (res,) = _roundtrip(path, [struct.pack("<Q", len(msg)) + msg], compute)
    p, sig = eigen_decode(res["pressure"]), eigen_decode(res["stress"])
    assert p.shape == (16,) and sig.shape == (9, 16)
    be = NumpyPressureBackend()
    p_ref = pressure_field(frame, probes, 1.0, be)
    s_ref = stress_field(frame, probes, 1.0, be)
    print("listener: pressure", rel(p, p_ref), "stress", rel(sig.T.reshape(-1, 3, 3), s_ref))
    assert np.linalg.norm(p_ref) > 0
    assert rel(p, p_ref) < 1e-10
    assert rel(sig.T.reshape(-1, 3, 3), s_ref) < 1e-10


# ---- the C++ mirror -----------------------------------------------------------------------

PROBE_CASE = replace(PC.CASES["near"][0], reg=2e-3, eps=3e-5)
PROBE_RESULTS = [("stokeslet_pressure", "stokeslet_pressure"),
                 ("stresslet_pressure", "stresslet_pressure"),
                 ("oseen_tensor_contract_pressure", "oseen_pressure")]


@pytest.fixture(scope="module")
def probe_results(hip_lib_path, tmp_path_factory):
    """{label: (n_trg,) array} of one run of tests/pressure_probe.cpp, built with
    the host compiler the way test_gpu_cpp_mirror.py builds its probe."""
    from test_gpu_cpp_mirror import write_case, INCLUDE, LIBDIR
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("pressure_probe")
    exe, case, out = (str(tmp / n) for n in ("pressure_probe", "case.bin", "out.bin"))
    built = subprocess.run(
        [cxx, "-O2", "-std=c++17", "-I", INCLUDE, os.path.join(REPO, "tests", "pressure_probe.cpp"),
         "-L", LIBDIR, "-lskellyhip", "-Wl,-rpath," + LIBDIR, "-o", exe],
        capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    write_case(case, PROBE_CASE)
    r = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"pressure_probe failed ({r.returncode}): {r.stdout} {r.stderr}"
    flat = np.fromfile(out, np.float64)
    n_trg = len(PROBE_CASE.r_trg)
    assert flat.size == n_trg * len(PROBE_RESULTS)
    return {label: flat[i * n_trg:(i + 1) * n_trg] for i, (label, _) in enumerate(PROBE_RESULTS)}


@pytest.mark.parametrize("label,kernel", PROBE_RESULTS)
def test_cpp_mirror_is_the_python_host_form(ska, probe_results, label, kernel):
    got = probe_results[label]
    ref, A = PR.reference("near_reg2e-3_eps3e-5_probe", kernel, PROBE_CASE)
    judge(f"{kernel} C++ {label}", got, ref, A, PR.bound(A, PROBE_CASE.n_src, 1, kernel))
    want = EVALUATE[kernel](ska, PROBE_CASE)
    assert np.array_equal(got, want), \
        f"{label}: {np.count_nonzero(got != want)} entries differ from the Python host form"
