"""GPU tests of the analytic velocity-gradient kernels (csrc/pair_functors.hpp:
StokesletGrad, StressletGrad, RotletGrad through the shared pair driver).

Expected values are the numpy closed forms of tests/test_gradient_cpu.py,
gate REL_TOL = 1e-10 norm-relative (the parity bar of test_gpu_parity.py).
Sizes follow the driver's paths: TILE = 512 sources per LDS tile, unroll 2,
256-thread blocks with up to 2 targets a thread, a source slice per 2048
sources when the target grid is small."""

import os
import struct

import msgpack
import numpy as np
import pytest

from test_gradient_cpu import (np_stokeslet_grad, np_stresslet_grad, np_oseen_grad,
                               np_rotlet_grad, central_difference, curl, far_probes)

pytestmark = pytest.mark.gpu

REL_TOL = 1e-10
ETA = 1.3


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


def gpu_grad(ska, kernel, r_src, f, r_trg, eta=ETA):
    if kernel == "stokeslet":
        return ska.stokeslet_grad(r_src, f, r_trg, eta)
    if kernel == "stresslet":
        return ska.stresslet_grad(r_src, f, r_trg, eta)
    if kernel == "oseen":
        return ska.oseen_contract_grad(r_src, r_trg, f, eta)
    return ska.rotlet_grad(r_src, r_trg, f, eta)


def np_grad(kernel, r_src, f, r_trg, eta=ETA):
    if kernel == "stokeslet":
        return np_stokeslet_grad(r_src, f, r_trg, eta)
    if kernel == "stresslet":
        return np_stresslet_grad(r_src, f, r_trg, eta)
    if kernel == "oseen":
        return np_oseen_grad(r_src, r_trg, f, eta)
    return np_rotlet_grad(r_src, r_trg, f, eta)


def gpu_velocity(ska, kernel, r_src, f, r_trg, eta=ETA):
    if kernel == "stokeslet":
        return ska.stokeslet_direct_gpu(r_src, None, r_trg, f, None, eta)
    if kernel == "stresslet":
        return ska.stresslet_direct_gpu(None, r_src, r_trg, None, f, eta)
    if kernel == "oseen":
        return ska.oseen_contract_direct_gpu(r_src, r_trg, f, eta)
    return ska.rotlet_gpu(r_src, r_trg, f, eta)


_clouds = {}


def cloud(kernel, n_src, n_trg, golden_dir):
    """(r_src, f, r_trg) of one case, made once. (1229, 743) is the committed
    kernel-test recipe; the others are uniform in [-1, 1]^3."""
    key = (kernel, n_src, n_trg)
    if key not in _clouds:
        fdim = 9 if kernel == "stresslet" else 3
        if (n_src, n_trg) == (1229, 743):
            g = np.load(os.path.join(golden_dir, "kernel_test_1229x743.npz"))
            assert float(g["eta"]) == ETA
            _clouds[key] = (g["r_src"], g["f9" if fdim == 9 else "f3"], g["r_trg"])
        else:
            rng = np.random.default_rng(1000 * n_src + n_trg)
            _clouds[key] = (rng.uniform(-1, 1, (n_src, 3)), rng.uniform(-1, 1, (n_src, fdim)),
                            rng.uniform(-1, 1, (n_trg, 3)))
    return _clouds[key]


_refs = {}


def reference(kernel, n_src, n_trg, golden_dir):
    key = (kernel, n_src, n_trg)
    if key not in _refs:
        r_src, f, r_trg = cloud(kernel, n_src, n_trg, golden_dir)
        _refs[key] = np_grad(kernel, r_src, f, r_trg)
        _refs[key].setflags(write=False)
    return _refs[key]


# (n_src, n_trg): path
#   (1, 1)        degenerate single pair
#   (515, 1)      second LDS tile, unrolled group + scalar tail, 1 target/thread
#   (1229, 743)   committed clouds; 2 targets/thread, partial last block
#   (2051, 1027)  largest targets-per-thread variant, two source slices,
#                 9-wide partial reduce
#   (4099, 5)     three slices
SIZES = [(1, 1), (515, 1), (1229, 743), (2051, 1027), (4099, 5)]
CASES = [(k, s) for k in ("stokeslet", "stresslet", "oseen") for s in SIZES] + \
        [("rotlet", s) for s in (SIZES[0], SIZES[2], SIZES[4])]


@pytest.mark.parametrize("kernel,size", CASES,
                         ids=[f"{k}-{s[0]}x{s[1]}" for k, s in CASES])
def test_gradient_matches_closed_form(ska, golden_dir, kernel, size):
    r_src, f, r_trg = cloud(kernel, *size, golden_dir)
    G = gpu_grad(ska, kernel, r_src, f, r_trg)
    ref = reference(kernel, *size, golden_dir)
    assert G.shape == (size[1], 3, 3)
    err = rel(G, ref)
    print(kernel, size, "rel", err)
    assert np.all(np.isfinite(G)) and err < REL_TOL, err


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen", "rotlet"])
def test_coincident_points(ska, golden_dir, kernel):
    """Sources acting on themselves, with duplicated points: r^2 == 0 pairs
    drop out for stokeslet/stresslet/oseen and regularize for the rotlet."""
    g = np.load(os.path.join(golden_dir, "edge_selfdup.npz"))
    r, eta = g["r"], float(g["eta"])
    d2 = ((r[:, None, :] - r[None, :, :]) ** 2).sum(-1)
    assert (d2 == 0).sum() > len(r)  # duplicates beyond the diagonal
    f = g["f9"] if kernel == "stresslet" else g["f3"]
    G = gpu_grad(ska, kernel, r, f, r, eta)
    assert np.all(np.isfinite(G))
    err = rel(G, np_grad(kernel, r, f, r, eta))
    print(kernel, "selfdup rel", err)
    assert err < REL_TOL, err


def test_oseen_regularized_branch(ska, golden_dir):
    """Targets ~3e-6 from their sources: under epsilon_distance, the
    derivative of the regularized expression."""
    g = np.load(os.path.join(golden_dir, "refpy_small.npz"))
    eta = float(g["eta"])
    src, rho, near = g["r_src"][:40], g["f3"][:40], g["near_trg"]
    dist = np.linalg.norm(near[:, None, :] - src[None, :, :], axis=2).min(axis=1)
    assert np.all(dist > 0) and np.all(dist < 1e-5)
    G = ska.oseen_contract_grad(src, near, rho, eta)
    ref = np_oseen_grad(src, near, rho, eta)
    assert rel(G, ref) < REL_TOL, rel(G, ref)
    # ... which is not the plain Stokeslet's gradient there
    assert rel(np_stokeslet_grad(src, rho, near, eta), ref) > 1.0


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen", "rotlet"])
def test_gradient_matches_differences_of_velocity_kernels(ska, kernel):
    """Cross-check against the velocity kernels, which are pinned to the
    reference: central differences at h = 1e-5, sources in [-1, 1]^3, 64
    targets on the sphere of radius 2.5. The closed forms agree to 1.7e-10 on
    this geometry; the gate of 1e-7 leaves room for another summation order,
    a wrong term is O(1)."""
    rng = np.random.default_rng(515)
    r_src = rng.uniform(-1, 1, (515, 3))
    f = rng.uniform(-1, 1, (515, 9 if kernel == "stresslet" else 3))
    v = rng.normal(size=(64, 3))
    r_trg = 2.5 * v / np.linalg.norm(v, axis=1)[:, None]
    G = gpu_grad(ska, kernel, r_src, f, r_trg)
    fd = central_difference(lambda p: gpu_velocity(ska, kernel, r_src, f, p), r_trg, h=1e-5)
    err = rel(G, fd)
    print(kernel, "vs differences of the velocity kernel", err)
    assert err < 1e-7, err


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet"])
def test_trace_free(ska, golden_dir, kernel):
    r_src, f, r_trg = cloud(kernel, 1229, 743, golden_dir)
    G = gpu_grad(ska, kernel, r_src, f, r_trg)
    tr = np.trace(G, axis1=1, axis2=2)
    print(kernel, "trace", np.linalg.norm(tr) / np.linalg.norm(G))
    assert np.linalg.norm(tr) < 1e-12 * np.linalg.norm(G)


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen", "rotlet"])
@pytest.mark.parametrize("size", [(1229, 743), (4099, 5)], ids=["single-slice", "split"])
def test_deterministic_and_fastpath_independent(ska, golden_dir, kernel, size):
    from skellysim_amd import _native
    r_src, f, r_trg = cloud(kernel, *size, golden_dir)
    a = gpu_grad(ska, kernel, r_src, f, r_trg)
    b = gpu_grad(ska, kernel, r_src, f, r_trg)
    assert np.array_equal(a, b)
    try:
        _native.set_pair_fastpath(0)
        off = gpu_grad(ska, kernel, r_src, f, r_trg)
        _native.set_pair_fastpath(2)
        on = gpu_grad(ska, kernel, r_src, f, r_trg)
    finally:
        _native.set_pair_fastpath(1)
    assert np.array_equal(off, on) and np.array_equal(off, a)


@pytest.mark.parametrize("kernel", ["stokeslet", "stresslet", "oseen", "rotlet"])
def test_device_and_host_forms_agree(ska, golden_dir, kernel):
    import torch
    r_src, f, r_trg = cloud(kernel, 1229, 743, golden_dir)
    dev = torch.device("cuda:0")
    ts, tf, tt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (r_src, f, r_trg))
    if kernel == "stokeslet":
        G = ska.stokeslet_grad_device(ts, tf, tt, ETA)
    elif kernel == "stresslet":
        G = ska.stresslet_grad_device(ts, tf, tt, ETA)
    elif kernel == "oseen":
        G = ska.oseen_contract_grad_device(ts, tt, tf, ETA)
    else:
        G = ska.rotlet_grad_device(ts, tt, tf, ETA)
    torch.cuda.synchronize()
    assert G.shape == (743, 3, 3)
    assert np.array_equal(G.cpu().numpy(), gpu_grad(ska, kernel, r_src, f, r_trg))


def test_flows_gradient_composition(ska):
    """flows.velocity_gradient_at_targets sums the same terms as
    velocity_at_targets; checked against the closed forms."""
    import torch
    from skellysim_amd.flows import velocity_gradient_at_targets, vorticity_from_gradient
    rng = np.random.default_rng(8)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fib = dict(r_src=rng.uniform(-1, 1, (70, 3)), forces=rng.uniform(-1, 1, (70, 3)),
               weights=rng.uniform(0.1, 0.2, 70))
    shell = dict(node_pos=rng.uniform(-1, 1, (90, 3)), node_normal=rng.uniform(-1, 1, (90, 3)),
                 density=rng.uniform(-1, 1, (90, 3)))
    bodies = dict(node_pos=rng.uniform(-1, 1, (50, 3)), node_normals=rng.uniform(-1, 1, (50, 3)),
                  densities=rng.uniform(-1, 1, (50, 3)), centers=rng.uniform(-1, 1, (2, 3)),
                  forces=rng.uniform(-1, 1, (2, 3)), torques=rng.uniform(-1, 1, (2, 3)))
    r_trg = rng.uniform(-1, 1, (33, 3))
    G = velocity_gradient_at_targets(
        t(r_trg), ETA, fiber={k: t(v) for k, v in fib.items()},
        shell={k: t(v) for k, v in shell.items()}, bodies={k: t(v) for k, v in bodies.items()})
    torch.cuda.synchronize()
    dl = lambda n, d: 2.0 * ETA * np.einsum("ni,nj->nij", n, d).reshape(-1, 9)
    ref = np_stokeslet_grad(fib["r_src"], fib["forces"] * fib["weights"][:, None], r_trg, ETA)
    ref += np_stresslet_grad(shell["node_pos"], dl(shell["node_normal"], shell["density"]),
                             r_trg, ETA)
    ref += np_stresslet_grad(bodies["node_pos"], dl(bodies["node_normals"], bodies["densities"]),
                             r_trg, ETA)
    ref += np_stokeslet_grad(bodies["centers"], bodies["forces"], r_trg, ETA)
    ref += np_rotlet_grad(bodies["centers"], r_trg, bodies["torques"], ETA)
    assert rel(G.cpu().numpy(), ref) < REL_TOL
    assert np.array_equal(vorticity_from_gradient(G).cpu().numpy(), curl(G.cpu().numpy()))


def test_listener_gradient_field_hip(tmp_path, hip_lib_path):
    """Frame level on the product backend: velocity_gradient_field against
    central differences of velocity_field (h = 1e-5, probes at least 0.5 from
    every source node, where truncation is ~10 (h/r)^2 = 4e-9; gate 1e-6), and
    the vortex-line request with "analytic": true, whose val is the curl of
    that gradient at the returned points."""
    from skellysim_amd.fiber_fd import FiberFD
    from skellysim_amd.system_fd import SystemFD, HipBackend
    from skellysim_amd.trajectory import TrajectoryWriter
    from skellysim_amd.listener import (Trajectory, eigen_decode, velocity_field,
                                        velocity_gradient_field)
    from test_listener import _ndencode, _roundtrip

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
    G = velocity_gradient_field(frame, probes, 1.0, compute)
    fd = central_difference(lambda p: velocity_field(frame, p, 1.0, compute), probes, h=1e-5)
    err = rel(G, fd)
    print("frame gradient vs central differences", err)
    assert err < 1e-6, err

    cmd = {
        "frame_no": 0,
        "evaluator": "GPU",
        "streamlines": {"dt_init": 0.1, "t_final": 1.0, "abs_err": 1e-10,
                        "rel_err": 1e-6, "back_integrate": True,
                        "x0": np.zeros((0, 3))},
        "vortexlines": {"dt_init": 0.05, "t_final": 0.2, "abs_err": 1e-10,
                        "rel_err": 1e-8, "back_integrate": False,
                        "x0": np.array([[0.6, 0.2, 0.4]]), "analytic": True},
        "velocity_field": {"x": np.zeros((0, 3))},
    }
    msg = msgpack.packb(cmd, default=_ndencode)
    (res,) = _roundtrip(path, [struct.pack("<Q", len(msg)) + msg], compute)
    (vl,) = res["vortexlines"]
    xp, val = eigen_decode(vl["x"]), eigen_decode(vl["val"])
    assert len(xp) > 2
    w = curl(velocity_gradient_field(frame, xp, 1.0, compute))
    assert rel(val, w) < 1e-10
