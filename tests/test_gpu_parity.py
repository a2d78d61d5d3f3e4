"""GPU parity tests: the HIP kernels against the CPU oracle / committed golden
fixtures on identical clouds.

Bar: <= 1e-10 RELATIVE velocity error vs the CPU reference path
(stricter than the reference's own 5e-9 absolute Frobenius gate,
tests/core/kernel_test.cpp:92, which is also asserted)."""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-10  # BASELINE.json north_star parity bar
ABS_TOL = 5e-9   # reference kernel_test.cpp:92 gate


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "kernel_test_1229x743.npz"))


def test_stokeslet_golden_recipe(ska, golden):
    """Reference parity recipe: 1229 x 743, eta=1.3 (kernel_test.cpp:25-27)."""
    eta = float(golden["eta"])
    u = ska.stokeslet_direct_gpu(golden["r_src"], None, golden["r_trg"], golden["f3"], None, eta)
    assert rel(u, golden["u_stokeslet"]) < REL_TOL
    assert np.linalg.norm(u - golden["u_stokeslet"]) < ABS_TOL


def test_stresslet_golden_recipe(ska, golden):
    eta = float(golden["eta"])
    u = ska.stresslet_direct_gpu(None, golden["r_src"], golden["r_trg"], None, golden["f9"], eta)
    assert rel(u, golden["u_stresslet"]) < REL_TOL
    assert np.linalg.norm(u - golden["u_stresslet"]) < ABS_TOL


def test_oseen_golden_recipe(ska, golden):
    eta = float(golden["eta"])
    u = ska.oseen_contract_direct_gpu(golden["r_src"], golden["r_trg"], golden["f3"], eta)
    assert rel(u, golden["u_oseen"]) < REL_TOL


def test_rotlet_golden_recipe(ska, golden):
    eta = float(golden["eta"])
    u = ska.rotlet_gpu(golden["r_src"][:37], golden["r_trg"], golden["f3"][:37], eta)
    assert rel(u, golden["u_rotlet"]) < REL_TOL


def test_oseen_near_branch(ska, golden_dir):
    """Regularized branch (dr <= eps): targets displaced ~3e-6 from sources."""
    g = np.load(os.path.join(golden_dir, "refpy_small.npz"))
    eta = float(g["eta"])
    u = ska.oseen_contract_direct_gpu(g["r_src"][:40], g["near_trg"], g["f3"][:40], eta)
    assert rel(u, g["u_oseen_near"]) < REL_TOL


def test_edge_selfdup(ska, golden_dir):
    """Coincident points: src==trg self-interaction and duplicated points must
    contribute zero (stokeslet/stresslet/oseen) / regularized (rotlet)."""
    g = np.load(os.path.join(golden_dir, "edge_selfdup.npz"))
    eta = float(g["eta"])
    u = ska.stokeslet_direct_gpu(g["r"], None, g["r"], g["f3"], None, eta)
    assert np.all(np.isfinite(u)) and rel(u, g["u_stokeslet"]) < REL_TOL
    u = ska.stresslet_direct_gpu(None, g["r"], g["r"], None, g["f9"], eta)
    assert np.all(np.isfinite(u)) and rel(u, g["u_stresslet"]) < REL_TOL
    u = ska.oseen_contract_direct_gpu(g["r"], g["r"], g["f3"], eta)
    assert np.all(np.isfinite(u)) and rel(u, g["u_oseen"]) < REL_TOL
    u = ska.rotlet_gpu(g["r"], g["r"], g["f3"], eta)
    assert np.all(np.isfinite(u)) and rel(u, g["u_rotlet"]) < REL_TOL


@pytest.mark.parametrize("n_src,n_trg", [
    (1, 1), (1, 777), (513, 1), (512, 1024), (1229, 743),
    (4096, 4096), (5000, 3000), (511, 255), (1025, 257),
])
def test_stokeslet_sizes_vs_oracle(ska, oracle_mod, n_src, n_trg):
    """Tile/remainder coverage: sizes off multiples of TILE=512 and
    BLOCK*TPT."""
    rng = np.random.default_rng(n_src * 7 + n_trg)
    r_src = rng.uniform(-1, 1, (n_src, 3))
    f_src = rng.uniform(-1, 1, (n_src, 3))
    r_trg = rng.uniform(-1, 1, (n_trg, 3))
    u = ska.stokeslet_direct_gpu(r_src, None, r_trg, f_src, None, 1.1)
    ref = oracle_mod.stokeslet(r_src, f_src, r_trg, 1.1)
    assert rel(u, ref) < REL_TOL


@pytest.mark.parametrize("n_src,n_trg", [(1, 1), (512, 1024), (1229, 743), (2048, 513)])
def test_stresslet_sizes_vs_oracle(ska, oracle_mod, n_src, n_trg):
    rng = np.random.default_rng(n_src + n_trg)
    r_src = rng.uniform(-1, 1, (n_src, 3))
    f9 = rng.uniform(-1, 1, (n_src, 9))
    r_trg = rng.uniform(-1, 1, (n_trg, 3))
    u = ska.stresslet_direct_gpu(None, r_src, r_trg, None, f9, 0.8)
    ref = oracle_mod.stresslet(r_src, f9, r_trg, 0.8)
    assert rel(u, ref) < REL_TOL


@pytest.mark.parametrize("n_src,n_trg", [
    (20000, 8192),    # split path: 32 target blocks -> ~10 source slices
    (100000, 4096),   # deeper split
    (5000, 100),      # tiny targets, few slices
])
def test_source_split_path_vs_oracle(ska, oracle_mod, n_src, n_trg):
    """Small-target launches take the source-split (split-K) path; results
    must still match the oracle and be deterministic."""
    rng = np.random.default_rng(n_src ^ n_trg)
    r_src = rng.uniform(-1, 1, (n_src, 3))
    f_src = rng.uniform(-1, 1, (n_src, 3))
    r_trg = rng.uniform(-1, 1, (n_trg, 3))
    u = ska.stokeslet_direct_gpu(r_src, None, r_trg, f_src, None, 1.3)
    ref = oracle_mod.stokeslet(r_src, f_src, r_trg, 1.3)
    assert rel(u, ref) < REL_TOL
    u2 = ska.stokeslet_direct_gpu(r_src, None, r_trg, f_src, None, 1.3)
    assert np.array_equal(u, u2)
    f9 = rng.uniform(-1, 1, (n_src, 9))
    u9 = ska.stresslet_direct_gpu(None, r_src, r_trg, None, f9, 1.3)
    ref9 = oracle_mod.stresslet(r_src, f9, r_trg, 1.3)
    assert rel(u9, ref9) < REL_TOL


def test_empty_sources_and_targets(ska):
    r = np.random.default_rng(0).uniform(-1, 1, (16, 3))
    f = np.ones((16, 3))
    u = ska.stokeslet_direct_gpu(np.empty((0, 3)), None, r, np.empty((0, 3)), None, 1.0)
    assert u.shape == (16, 3) and np.all(u == 0)
    u = ska.stokeslet_direct_gpu(r, None, np.empty((0, 3)), f, None, 1.0)
    assert u.shape == (0, 3)


def test_stresslet_normal_density_vs_oracle(ska, oracle_mod):
    """kernels::stresslet_times_normal_times_density (kernels.cpp:307-334):
    host and device paths vs oracle, incl. the i==j skip and duplicates."""
    rng = np.random.default_rng(41)
    n = 2000
    r = rng.uniform(-1, 1, (n, 3))
    r[100:117] = r[0:17]  # duplicated points (d==0 mask must equal i==j skip)
    nrm = rng.uniform(-1, 1, (n, 3))
    rho = rng.uniform(-1, 1, (n, 3))
    out = ska.stresslet_times_normal_times_density(r, nrm, rho)
    ref = oracle_mod.stresslet_times_normal_times_density(r, nrm, rho)
    assert np.all(np.isfinite(out)) and rel(out, ref) < REL_TOL
    # near-regularized branch: points separated by ~3e-6 < eps
    r2 = np.vstack([r[:50], r[:50] + 3e-6])
    out2 = ska.stresslet_times_normal_times_density(r2, np.vstack([nrm[:50]] * 2),
                                                    np.vstack([rho[:50]] * 2))
    ref2 = oracle_mod.stresslet_times_normal_times_density(r2, np.vstack([nrm[:50]] * 2),
                                                           np.vstack([rho[:50]] * 2))
    assert rel(out2, ref2) < REL_TOL
    # device form matches host form
    import torch
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(a).to(dev)
    out3 = ska.stresslet_normal_density_device(T(r), T(nrm), T(rho))
    torch.cuda.synchronize()
    assert np.array_equal(out3.cpu().numpy(), out)


def test_stresslet_times_normal_dense_vs_oracle(ska, oracle_mod):
    """Dense stresslet_times_normal builder (kernels.cpp:264-287) vs the
    numpy restatement, plus the contraction identity
    Snormal @ rho == stresslet_times_normal_times_density."""
    import torch
    rng = np.random.default_rng(61)
    n = 300
    r = rng.uniform(-1, 1, (n, 3))
    nrm = rng.uniform(-1, 1, (n, 3))
    rho = rng.uniform(-1, 1, (n, 3))
    dev = torch.device("cuda:0")
    S = ska.stresslet_times_normal_device(torch.from_numpy(r).to(dev),
                                          torch.from_numpy(nrm).to(dev))
    torch.cuda.synchronize()
    Sh = S.cpu().numpy()
    ref = oracle_mod.np_stresslet_times_normal(r, nrm)
    assert rel(Sh, ref) < REL_TOL
    contr = (Sh @ rho.reshape(-1)).reshape(-1, 3)
    sdn = oracle_mod.stresslet_times_normal_times_density(r, nrm, rho)
    assert rel(contr, sdn) < 1e-12


def test_oseen_tensor_batched_vs_oracle(ska, oracle_mod):
    """Batched per-fiber self-stokeslet dense build (kernels.cpp:146-195 via
    fiber_finite_difference.cpp:56), incl. a near-regularized fiber."""
    import torch
    rng = np.random.default_rng(51)
    nf, n = 40, 32
    pts = rng.uniform(-1, 1, (nf, n, 3))
    pts[3, 10] = pts[3, 11] + 4e-6  # regularized branch inside fiber 3
    dev = torch.device("cuda:0")
    G = ska.oseen_tensor_batched_device(torch.from_numpy(pts).to(dev), eta=1.3)
    torch.cuda.synchronize()
    Gh = G.cpu().numpy()
    for f in [0, 3, nf - 1]:
        ref = oracle_mod.oseen_tensor(pts[f], 1.3)
        assert rel(Gh[f], ref) < REL_TOL
    # diagonal blocks exactly zero
    for i in range(n):
        assert np.all(Gh[0, 3 * i: 3 * i + 3, 3 * i: 3 * i + 3] == 0.0)


def test_dropin_impl_scaling(ska, oracle_mod):
    """The drop-in *_direct_gpu_impl entry points include 1/(8 pi) but NOT the
    /eta division (reference kernels.cpp:358,365 divide afterwards)."""
    import ctypes
    from skellysim_amd import _native
    rng = np.random.default_rng(5)
    n_src, n_trg = 700, 350
    r_src = np.ascontiguousarray(rng.uniform(-1, 1, (n_src, 3)))
    f_src = np.ascontiguousarray(rng.uniform(-1, 1, (n_src, 3)))
    r_trg = np.ascontiguousarray(rng.uniform(-1, 1, (n_trg, 3)))
    u = np.zeros((n_trg, 3))
    DP = ctypes.POINTER(ctypes.c_double)
    _native.lib().stokeslet_direct_gpu_impl(
        r_src.ctypes.data_as(DP), f_src.ctypes.data_as(DP), n_src,
        r_trg.ctypes.data_as(DP), u.ctypes.data_as(DP), n_trg)
    ref = oracle_mod.stokeslet(r_src, f_src, r_trg, 1.0)  # eta=1 == unscaled by eta
    assert rel(u, ref) < REL_TOL


def test_determinism_bitwise(ska, golden):
    """Fixed-order accumulation: repeated runs are bit-identical."""
    eta = float(golden["eta"])
    u1 = ska.stokeslet_direct_gpu(golden["r_src"], None, golden["r_trg"], golden["f3"], None, eta)
    u2 = ska.stokeslet_direct_gpu(golden["r_src"], None, golden["r_trg"], golden["f3"], None, eta)
    assert np.array_equal(u1, u2)


def test_device_api_matches_host_api(ska, golden):
    """The torch device-tensor path equals the host-pointer path bitwise."""
    import torch
    eta = float(golden["eta"])
    dev = torch.device("cuda:0")
    r_src = torch.from_numpy(golden["r_src"]).to(dev)
    f_src = torch.from_numpy(golden["f3"]).to(dev)
    r_trg = torch.from_numpy(golden["r_trg"]).to(dev)
    u_dev = ska.stokeslet_device(r_src, f_src, r_trg, eta)
    torch.cuda.synchronize()
    u_host = ska.stokeslet_direct_gpu(golden["r_src"], None, golden["r_trg"],
                                      golden["f3"], None, eta)
    assert np.array_equal(u_dev.cpu().numpy(), u_host)


# (host function, device function, source-strength key) of the kernels that
# take (r_src, strength, r_trg, eta) and of those that take
# (r_src, r_trg, density, eta, reg, eps); the last pair has its own signature.
HOST_DEVICE_PAIRS = {
    "stokeslet": ("stokeslet_direct_gpu", "stokeslet_device", "f3"),
    "stresslet": ("stresslet_direct_gpu", "stresslet_device", "f9"),
    "oseen_contract": ("oseen_contract_direct_gpu", "oseen_contract_device", "f3"),
    "rotlet": ("rotlet_gpu", "rotlet_device", "f3"),
    "stokeslet_grad": ("stokeslet_grad", "stokeslet_grad_device", "f3"),
    "stresslet_grad": ("stresslet_grad", "stresslet_grad_device", "f9"),
    "oseen_contract_grad": ("oseen_contract_grad", "oseen_contract_grad_device", "f3"),
    "rotlet_grad": ("rotlet_grad", "rotlet_grad_device", "f3"),
    "stresslet_normal_density": ("stresslet_times_normal_times_density",
                                 "stresslet_normal_density_device", None),
}


@pytest.mark.parametrize("slices", [0, 3], ids=["planned", "slices3"])
@pytest.mark.parametrize("kernel", list(HOST_DEVICE_PAIRS))
def test_device_api_matches_host_api_every_kernel(ska, golden, kernel, slices):
    """test_device_api_matches_host_api for every kernel, with non-default
    reg and eps, under the planner's slice count and under a forced one."""
    import torch
    from skellysim_amd import _native
    host_name, dev_name, fkey = HOST_DEVICE_PAIRS[kernel]
    host_fn, dev_fn = getattr(ska, host_name), getattr(ska, dev_name)
    eta = float(golden["eta"])
    dev = torch.device("cuda:0")

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    r_src, r_trg = golden["r_src"], golden["r_trg"]
    _native.set_pair_slices(slices)
    try:
        if kernel == "stresslet_normal_density":
            # one point set: sources are the targets
            nrm, rho = golden["f3"], golden["f9"][:, 2:5]
            out_dev = dev_fn(t(r_src), t(nrm), t(rho), reg=2e-3, epsilon_distance=3e-5)
            out_host = host_fn(r_src, nrm, rho, reg=2e-3, epsilon_distance=3e-5)
        elif kernel in ("stokeslet", "stresslet"):
            f = golden[fkey]
            out_dev = dev_fn(t(r_src), t(f), t(r_trg), eta)
            if kernel == "stokeslet":  # Evaluator signature: (r_sl, r_dl, r_trg, f_sl, f_dl)
                out_host = host_fn(r_src, None, r_trg, f, None, eta)
            else:
                out_host = host_fn(None, r_src, r_trg, None, f, eta)
        elif kernel in ("stokeslet_grad", "stresslet_grad"):
            f = golden[fkey]
            out_dev = dev_fn(t(r_src), t(f), t(r_trg), eta)
            out_host = host_fn(r_src, f, r_trg, eta)
        else:
            f = golden[fkey]
            out_dev = dev_fn(t(r_src), t(r_trg), t(f), eta, 2e-3, 3e-5)
            out_host = host_fn(r_src, r_trg, f, eta, 2e-3, 3e-5)
        torch.cuda.synchronize()
    finally:
        _native.set_pair_slices(0)
    assert out_dev.shape == out_host.shape
    assert np.isfinite(out_host).all() and np.abs(out_host).max() > 0
    assert np.array_equal(out_dev.cpu().numpy(), out_host)


@pytest.mark.parametrize("dev_name,width", [("stokeslet_device", (3,)),
                                            ("stokeslet_grad_device", (3, 3))])
def test_device_out_argument_is_validated(ska, golden, dev_name, width):
    """out= must be a contiguous float64 CUDA tensor of the result's size:
    anything else raises instead of being written through; a valid one is
    filled, returned, and equals the allocating call bitwise."""
    import torch
    dev = torch.device("cuda:0")
    fn = getattr(ska, dev_name)
    eta = float(golden["eta"])
    args = [torch.from_numpy(golden[k]).to(dev) for k in ("r_src", "f3", "r_trg")]
    n_trg = len(golden["r_trg"])
    ref = fn(*args, eta)

    transposed = torch.empty(width[::-1] + (n_trg,), dtype=torch.float64, device=dev)
    transposed = transposed.permute(*range(len(width), -1, -1))
    assert transposed.shape == (n_trg,) + width and not transposed.is_contiguous()
    with pytest.raises(ValueError):
        fn(*args, eta, out=transposed)
    with pytest.raises(ValueError):
        fn(*args, eta, out=torch.empty((n_trg - 1,) + width, dtype=torch.float64, device=dev))

    out = torch.full((n_trg,) + width, float("nan"), dtype=torch.float64, device=dev)
    assert fn(*args, eta, out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_large_cloud_property_checks(ska):
    """At a size where the oracle would be slow, check size-independent
    properties instead: linearity in f and 1/eta scaling (SURVEY §8c tier)."""
    rng = np.random.default_rng(11)
    n = 60_000
    r_src = rng.uniform(-1, 1, (n, 3))
    f = rng.uniform(-1, 1, (n, 3))
    g = rng.uniform(-1, 1, (n, 3))
    r_trg = rng.uniform(-1, 1, (n, 3))
    u_sum = ska.stokeslet_direct_gpu(r_src, None, r_trg, f + g, None, 1.0)
    u_f = ska.stokeslet_direct_gpu(r_src, None, r_trg, f, None, 1.0)
    u_g = ska.stokeslet_direct_gpu(r_src, None, r_trg, g, None, 1.0)
    assert rel(u_sum, u_f + u_g) < 1e-12
    u_eta = ska.stokeslet_direct_gpu(r_src, None, r_trg, f, None, 4.0)
    assert rel(u_f, 4.0 * u_eta) < 1e-14


def test_fp64_peak_helper(ska):
    import ctypes
    from skellysim_amd import _native
    out = ctypes.c_double()
    rc = _native.lib().skelly_fp64_peak_tflops(ctypes.byref(out))
    assert rc == 0
    # MI355X fp64 vector peak is ~78.6 TF; accept a broad sanity band
    assert 20.0 < out.value < 120.0, f"measured fp64 peak {out.value} TF"
