"""Every pair kernel and both dense builders, per target and per component,
against the longdouble references of tests/pair_reference.py:

    |out - ref| <= bound(A, n_src, n_slices, kernel)        elementwise,

with A the condition sum of the entry and the bound from rounding analysis and
the measured v_rsq_f64 seed (pair_reference.py, profiles/pair_accuracy.md); an
entry with A == 0 has to be exactly 0. The norm-relative tests
(test_gpu_parity.py and the others at REL_TOL = 1e-10) cannot see an error in
the 11th to 15th digit of one target; this file can.

Cases (tests/pair_cases.py, the smallest shapes that reach each mechanism):
  pair_*      1, 2, 3, 5 sources on 257 targets: the bound is K_ops u + P E_RSQ
              and little else (460 u for the stokeslet, 8192 u is 2^-40), which
              is what catches a wrong fold, constant or refinement;
  driver_*    131 sources on 1, 513, 1025 targets (every targets-a-thread
              build) in 1 and 3 forced slices, and 1300 x 1100;
  near        targets on, 3e-6 from and 1e-4 from a source;
  scale_*     the 131-source cloud times 2^-10 and 2^10, reg and eps at their
              defaults or scaled along, and translated by (1000, -1000, 500);
  threshold_* pairs at eps (1 +- 2^-20) and eps (1 +- 2^-10), default and
              other reg and eps; reg = 0 on coincident points.
Each case runs with the fast path forced on (twice) and off under its forced
slice count (sliced() of test_gpu_pair_slices.py); the bound is applied to
the result of each mode. Every run prints its largest |out - ref| / (u A)."""

import numpy as np
import pytest

import pair_cases as PC
import pair_reference as R
from test_gpu_pair_slices import sliced

pytestmark = pytest.mark.gpu

LD = R.LD


@pytest.fixture(scope="module")
def ska(hip_lib_path):
    import skellysim_amd
    return skellysim_amd


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _normal_density(ska, c):
    """The functor on targets of its own: the device form (the host form is
    the self form)."""
    import torch
    out = ska.stresslet_normal_density_device(_t(c.r_src), _t(c.nrm), _t(c.f3), _t(c.r_trg),
                                              reg=c.reg, epsilon_distance=c.eps)
    torch.cuda.synchronize()
    return out.cpu().numpy()


EVALUATE = {
    "stokeslet": lambda ska, c: ska.stokeslet_direct_gpu(c.r_src, None, c.r_trg, c.f3, None,
                                                         c.eta),
    "stresslet": lambda ska, c: ska.stresslet_direct_gpu(None, c.r_src, c.r_trg, None, c.f9,
                                                         c.eta),
    "oseen": lambda ska, c: ska.oseen_contract_direct_gpu(c.r_src, c.r_trg, c.f3, c.eta, c.reg,
                                                          c.eps),
    "rotlet": lambda ska, c: ska.rotlet_gpu(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
    "normal_density": _normal_density,
    "stokeslet_grad": lambda ska, c: ska.stokeslet_grad(c.r_src, c.f3, c.r_trg, c.eta),
    "stresslet_grad": lambda ska, c: ska.stresslet_grad(c.r_src, c.f9, c.r_trg, c.eta),
    "oseen_grad": lambda ska, c: ska.oseen_contract_grad(c.r_src, c.r_trg, c.f3, c.eta, c.reg,
                                                         c.eps),
    "rotlet_grad": lambda ska, c: ska.rotlet_grad(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
}


def judge(label, out, ref, A, limit):
    """Print the largest |out - ref| / (u A), then hold every entry to `limit`."""
    assert out.shape == ref.shape
    err = np.abs(out.astype(LD) - ref)
    pos = A > 0
    worst = R.excess(out, ref, A)
    cap = float((limit[pos] / (R.U * A[pos])).min()) if pos.any() else 0.0
    print(f"ACC {label}: max |out - ref| / (u A) = {worst:.2f}, bound {cap:.2f}")
    assert np.isfinite(out).all(), label
    assert (out[~pos] == 0).all(), f"{label}: entries with A == 0 must be exactly 0"
    bad = err > limit
    assert not bad.any(), (f"{label}: {np.count_nonzero(bad)} entries over the bound, worst "
                           f"{float((err[bad] / (R.U * A[bad])).max()):.2f} u A at "
                           f"{tuple(np.argwhere(bad)[0])}")


def run_case(ska, kernel, name, case, n_slices):
    ref, A = PC.reference(name, kernel, case)
    u_on, u_again, u_off = sliced(n_slices, lambda: EVALUATE[kernel](ska, case))
    assert np.array_equal(u_on, u_again, equal_nan=True), "two consecutive calls differ"
    limit = R.bound(A, case.n_src, min(n_slices, case.n_src), kernel)
    for mode, out in (("fastpath on", u_on), ("fastpath off", u_off)):
        judge(f"{kernel} {name} slices={n_slices} {mode}", out, ref, A, limit)


def _runs(cases, kernels):
    return [(k, n, s) for n, (_, slices) in cases.items() for s in slices for k in kernels]


@pytest.mark.parametrize("kernel,name,n_slices", _runs(PC.CASES, PC.KERNELS))
def test_kernel_within_bound(ska, kernel, name, n_slices):
    run_case(ska, kernel, name, PC.CASES[name][0], n_slices)


@pytest.mark.parametrize("kernel,name,n_slices", _runs(PC.THRESHOLD_CASES, PC.REGULARIZED))
def test_threshold_within_bound(ska, kernel, name, n_slices):
    """Pairs just either side of the eps^2 comparisons (`>` in oseen and its
    gradient, `<` in rotlet, its gradient and normal-density), and the near
    cloud again with other reg and eps."""
    run_case(ska, kernel, name, PC.THRESHOLD_CASES[name][0], n_slices)


@pytest.mark.parametrize("kernel,name,n_slices", _runs(PC.REG0_CASES, PC.MASKED_REGULARIZED))
def test_reg_zero_on_coincident_points(ska, kernel, name, n_slices):
    """reg = 0: a coincident pair has den = 0 and only the mask keeps it out."""
    run_case(ska, kernel, name, PC.REG0_CASES[name][0], n_slices)


# ---- dense builders: one pair an entry, nothing summed --------------------------

@pytest.mark.parametrize("nf,n", [(1, 1), (3, 7), (40, 32)])
def test_oseen_tensor_batched_within_bound(ska, nf, n):
    """(3, 7) is 147 pair threads, a ragged block; fiber 0 holds a pair 4e-6
    apart and the last fiber a coincident one (n >= 3)."""
    import torch
    pts = PC.fiber_points(nf, n)
    ref, A = R.oseen_tensor_batched(pts, 1.3)
    G = ska.oseen_tensor_batched_device(_t(pts), eta=1.3)
    torch.cuda.synchronize()
    judge(f"oseen_tensor {nf}x{n}", G.cpu().numpy(), ref, A, R.entry_bound(A, "oseen_tensor"))


@pytest.mark.parametrize("n", [1, 7, 300])
def test_stresslet_times_normal_within_bound(ska, n):
    """n >= 3 holds a pair 3.7e-6 apart (regularized) and a coincident one."""
    import torch
    c = PC.surface_points(n)
    ref, A = R.stresslet_times_normal(c.r_src, c.nrm)
    S = ska.stresslet_times_normal_device(_t(c.r_src), _t(c.nrm))
    torch.cuda.synchronize()
    judge(f"stresslet_times_normal {n}", S.cpu().numpy(), ref, A,
          R.entry_bound(A, "stresslet_times_normal"))
