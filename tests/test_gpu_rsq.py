"""The pair kernels' one fp64 primitive, measured: the raw v_rsq_f64 seed and
rsq_x2 (the seed plus one 3-op Newton step, R = 2/sqrt(x)) against a longdouble
1/sqrt(x), through skelly_rsq_accuracy_probe, which calls the very rsq_x2 the
functors call.

One launch of about 2^17 arguments: evenly spaced and random mantissas over
the two octaves [1, 2) and [2, 4) (both exponent parities), the values one ulp
either side of 1, 2 and 4, the exponents 2^+-{1, 40, 41, 300, 301}, values of
the size of reg^2 (2.5e-5 plus a small r^2), a few subnormals, and x = 0 and
x = inf, whose NaN the r == 0 mask and the fast path's NaN probe rely on.

The seed is a hardware instruction: its error is what this test measures
(printed per exponent parity, recorded in profiles/pair_accuracy.md), and
pair_reference.E_SEED is twice the recorded maximum."""

import ctypes

import numpy as np
import pytest

import pair_reference as R

pytestmark = pytest.mark.gpu

LD = R.LD


def arguments():
    rng = np.random.default_rng(2024)
    m = 2 ** 15
    even = 1.0 + np.arange(m) / m                       # [1, 2), spacing 2^-15
    rand = 1.0 + rng.integers(0, 2 ** 52, m) * 2.0 ** -52
    rand2 = 1.0 + rng.integers(0, 2 ** 52, m) * 2.0 ** -52
    octaves = np.concatenate([even, rand, 2.0 * even, 2.0 * rand2])
    edges = np.array([f(v, w) for v in (1.0, 2.0, 4.0)
                      for f, w in ((np.nextafter, 0.0), (lambda a, b: a, 0.0),
                                   (np.nextafter, 8.0))])
    mant = np.array([1.0, 1.5, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, rng.uniform(1, 2)])
    expo = np.concatenate([mant * 2.0 ** (s * e) for e in (1, 40, 41, 300, 301)
                           for s in (1, -1)])
    reg2 = 5e-3 * 5e-3 + np.concatenate([[0.0], 10.0 ** -rng.uniform(10, 20, 63)])
    subnormal = np.array([5e-324, 1e-320, 1e-310, 2.0 ** -1023, 2.0 ** -1042])
    special = np.array([0.0, np.inf])
    x = np.concatenate([octaves, edges, expo, reg2, subnormal, special])
    return x, len(x) - len(special) - len(subnormal), len(subnormal)


@pytest.fixture(scope="module")
def sweep(hip_lib_path):
    import torch
    from skellysim_amd import _native
    x, n_normal, n_sub = arguments()
    dev = torch.device("cuda:0")
    d_x = torch.from_numpy(x).to(dev)
    d_seed = torch.full_like(d_x, -1.0)
    d_ref = torch.full_like(d_x, -1.0)
    rc = _native.lib().skelly_rsq_accuracy_probe(
        ctypes.c_void_p(d_x.data_ptr()), ctypes.c_void_p(d_seed.data_ptr()),
        ctypes.c_void_p(d_ref.data_ptr()), len(x),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _native.check(rc, "rsq_accuracy_probe")
    torch.cuda.synchronize()
    return x, d_seed.cpu().numpy(), d_ref.cpu().numpy(), n_normal, n_sub


def errors(x, seed, refined):
    """|seed sqrt(x) - 1| and |refined sqrt(x) / 2 - 1| in longdouble."""
    root = np.sqrt(x.astype(LD))
    return np.abs(seed.astype(LD) * root - 1), np.abs(refined.astype(LD) * root / 2 - 1)


def test_sweep_size_and_coverage():
    x, n_normal, n_sub = arguments()
    assert 2 ** 17 <= len(x) < 2 ** 17 + 2 ** 10
    _, e = np.frexp(x[:n_normal])
    assert (e % 2 == 0).sum() >= 2 ** 16 and (e % 2 == 1).sum() >= 2 ** 16
    assert (x[n_normal:n_normal + n_sub] < np.finfo(float).tiny).all()


def test_seed_within_e_seed(sweep):
    x, seed, refined, n_normal, n_sub = sweep
    fin = n_normal + n_sub
    e_seed, _ = errors(x[:fin], seed[:fin], refined[:fin])
    _, e = np.frexp(x[:n_normal])
    for parity in (0, 1):
        sel = e % 2 == parity
        # frexp's exponent is one above the IEEE one: [1, 2) has e = 1
        print(f"e_seed, x in [{2 if parity == 0 else 1}, {4 if parity == 0 else 2}) * 4^k: "
              f"max {float(e_seed[:n_normal][sel].max()):.4e}")
    print(f"e_seed over the subnormals: max {float(e_seed[n_normal:].max()):.4e}")
    print(f"E_SEED = {float(R.E_SEED):.4e}")
    assert (e_seed <= R.E_SEED).all()


def test_rsq_x2_within_e_rsq(sweep):
    x, seed, refined, n_normal, n_sub = sweep
    fin = n_normal + n_sub
    _, e_ref = errors(x[:fin], seed[:fin], refined[:fin])
    print(f"rsq_x2: max |R sqrt(x)/2 - 1| = {float(e_ref.max() / R.U):.3f} u "
          f"(subnormals {float(e_ref[n_normal:].max() / R.U):.3f} u), "
          f"E_RSQ = {float(R.E_RSQ / R.U):.3f} u")
    assert (e_ref <= R.E_RSQ).all()


def test_seven_e_rsq_is_far_below_the_parity_bar():
    assert 7 * R.E_RSQ < 1e-12


def test_zero_and_infinity(sweep):
    """x = 0: the seed is +inf and rsq_x2 NaN (0 * inf), what the masks test
    for; x = inf: seed 0, rsq_x2 NaN again."""
    x, seed, refined, _, _ = sweep
    assert x[-2] == 0.0 and seed[-2] == np.inf and np.isnan(refined[-2])
    assert x[-1] == np.inf and seed[-1] == 0.0 and np.isnan(refined[-1])
