"""CPU tests of tests/pair_reference.py: the longdouble references have to be
right before they judge a kernel.

  * each agrees with the project's fp64 oracle (oracle/, or the np_* gradient
    closed forms of test_gradient_cpu.py) within bound() on the inputs of the
    GPU accuracy tests, so the fp64 oracle itself sits inside every bound that
    test_gpu_pair_accuracy.py applies to a kernel;
  * single pairs against mpmath at 50 digits: the velocities from formulas
    written out in mpmath, the gradients as mpmath's numerical derivative of
    those velocities;
  * central differences of the longdouble velocities converge to the
    longdouble gradients at second order;
  * A >= |ref|, and A == 0 exactly where every pair of a target is masked.
"""

import mpmath
import numpy as np
import pytest

import pair_cases as PC
import pair_reference as R
import test_gradient_cpu as G

LD = R.LD


# ---- against the fp64 oracle ---------------------------------------------------

def oracle_normal_density(o, c):
    """The oracle has the self form only: stack the targets behind the sources
    with zero normals and densities (they add exact zeros)."""
    if c.r_trg is c.r_src:
        return o.stresslet_times_normal_times_density(c.r_src, c.nrm, c.f3, c.reg, c.eps)
    pts = np.concatenate([c.r_src, c.r_trg])
    zero = np.zeros_like(c.r_trg)
    out = o.stresslet_times_normal_times_density(pts, np.concatenate([c.nrm, zero]),
                                                 np.concatenate([c.f3, zero]), c.reg, c.eps)
    return out[c.n_src:]


ORACLE = {
    "stokeslet": lambda o, c: o.stokeslet(c.r_src, c.f3, c.r_trg, c.eta),
    "stresslet": lambda o, c: o.stresslet(c.r_src, c.f9, c.r_trg, c.eta),
    "oseen": lambda o, c: o.oseen_contract(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
    "rotlet": lambda o, c: o.rotlet(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
    "normal_density": oracle_normal_density,
    "stokeslet_grad": lambda o, c: G.np_stokeslet_grad(c.r_src, c.f3, c.r_trg, c.eta),
    "stresslet_grad": lambda o, c: G.np_stresslet_grad(c.r_src, c.f9, c.r_trg, c.eta),
    "oseen_grad": lambda o, c: G.np_oseen_grad(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
    "rotlet_grad": lambda o, c: G.np_rotlet_grad(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
}

ORACLE_RUNS = ([(k, n) for n in PC.CASES for k in PC.KERNELS]
               + [(k, n) for n in PC.THRESHOLD_CASES for k in PC.REGULARIZED]
               + [(k, n) for n in PC.REG0_CASES for k in PC.MASKED_REGULARIZED])
ALL_CASES = {**PC.CASES, **PC.THRESHOLD_CASES, **PC.REG0_CASES}


@pytest.mark.parametrize("kernel,name", ORACLE_RUNS)
def test_reference_agrees_with_fp64_oracle(oracle_mod, kernel, name):
    case, _ = ALL_CASES[name]
    ref, A = PC.reference(name, kernel, case)
    out = ORACLE[kernel](oracle_mod, case)
    assert out.shape == ref.shape
    rows = np.ones(len(out), bool)
    if kernel == "normal_density" and name == "self_reg0":
        # the oracle skips i == j only: its reg = 0 rows of the duplicated
        # points are 0 * inf, where the kernels (and the reference) mask d == 0
        rows[[3, 4, 5, 40, 41, 42]] = False
        assert not np.isfinite(out[~rows]).any()
    assert np.isfinite(out[rows]).all()
    err = np.abs(out.astype(LD) - ref)
    print(f"{kernel} {name}: oracle max |out - ref| / (u A) = "
          f"{R.excess(out[rows], ref[rows], A[rows]):.1f}, bound "
          f"{float(R.bound(LD(1), case.n_src, 1, kernel) / R.U):.1f}")
    assert (err[rows] <= R.bound(A[rows], case.n_src, 1, kernel)).all()


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (40, 32)])
def test_oseen_tensor_reference_agrees_with_fp64_oracle(oracle_mod, shape):
    pts = PC.fiber_points(*shape)
    ref, A = R.oseen_tensor_batched(pts, 1.3)
    for f in range(shape[0]):
        out = oracle_mod.oseen_tensor(pts[f], 1.3)
        print(f"oseen_tensor {shape} fiber {f}: oracle max |out - ref| / (u A) = "
              f"{R.excess(out, ref[f], A[f]):.1f}")
        assert (np.abs(out.astype(LD) - ref[f]) <= R.entry_bound(A[f], "oseen_tensor")).all()


@pytest.mark.parametrize("n", [1, 7, 300])
def test_stresslet_times_normal_reference_agrees_with_fp64_oracle(oracle_mod, n):
    c = PC.surface_points(n)
    ref, A = R.stresslet_times_normal(c.r_src, c.nrm)
    out = oracle_mod.np_stresslet_times_normal(c.r_src, c.nrm)
    print(f"stresslet_times_normal {n}: oracle max |out - ref| / (u A) = "
          f"{R.excess(out, ref, A):.1f}")
    assert (np.abs(out.astype(LD) - ref) <= R.entry_bound(A, "stresslet_times_normal")).all()


# ---- against mpmath ------------------------------------------------------------

mpmath.mp.dps = 50
mpf = mpmath.mpf


def to_mp(x):
    """A longdouble as an mpf, exactly (two fp64 pieces)."""
    hi = float(x)
    return mpf(hi) + mpf(float(LD(x) - LD(hi)))


def mp_den(r2, reg, eps, rule):
    if rule == "plain":
        return r2
    if rule == "oseen":
        return r2 if r2 > mpf(eps) ** 2 else r2 + mpf(reg) ** 2
    return r2 + mpf(reg) ** 2 if r2 < mpf(eps) ** 2 else r2


def mp_velocity(kernel, c, t):
    """The velocity of source 0 of c at the mpmath point t."""
    s = [mpf(float(x)) for x in c.r_src[0]]
    f = [mpf(float(x)) for x in c.f3[0]]
    d = [t[k] - s[k] for k in range(3)]
    r2 = sum(x * x for x in d)
    pf = 1 / (8 * mpmath.pi * mpf(c.eta))
    rule, masked = {"stokeslet": ("plain", True), "stresslet": ("plain", True),
                    "oseen": ("oseen", True), "rotlet": ("rotlet", False),
                    "normal_density": ("rotlet", True)}[kernel]
    if masked and r2 == 0:
        return [mpf(0)] * 3
    y = 1 / mpmath.sqrt(mp_den(r2, c.reg, c.eps, rule))
    if kernel in ("stokeslet", "oseen"):
        fd = sum(f[k] * d[k] for k in range(3))
        return [pf * (y * f[i] + y ** 3 * fd * d[i]) for i in range(3)]
    if kernel == "stresslet":
        S = [[mpf(float(c.f9[0][3 * k + l])) for l in range(3)] for k in range(3)]
        C = sum(d[k] * S[k][l] * d[l] for k in range(3) for l in range(3))
        return [-3 * pf * y ** 5 * C * d[i] for i in range(3)]
    if kernel == "rotlet":
        return [pf * y ** 3 * (f[(i + 1) % 3] * d[(i + 2) % 3] - f[(i + 2) % 3] * d[(i + 1) % 3])
                for i in range(3)]
    n = [mpf(float(x)) for x in c.nrm[0]]
    dr, dn = sum(f[k] * d[k] for k in range(3)), sum(n[k] * d[k] for k in range(3))
    return [-3 / (4 * mpmath.pi) * dr * dn * y ** 5 * d[i] for i in range(3)]


def single_pairs():
    """One source, 20 targets: 14 anywhere, the four threshold distances, one
    coincident, one 3e-6 away."""
    c = PC.cloud(71, 1, 14)
    thr = PC.threshold_cloud(seed=72, n_src=1)
    trg = np.concatenate([c.r_trg, c.r_src + (thr.r_trg - thr.r_src), c.r_src,
                          c.r_src + np.array([[2e-6, -1e-6, 2e-6]])])
    return PC.replace(c, r_trg=trg)


VELOCITY_OF = {"stokeslet_grad": "stokeslet", "stresslet_grad": "stresslet",
               "oseen_grad": "oseen", "rotlet_grad": "rotlet"}
MP_TOL = 64 * LD(2.0) ** -64  # a few tens of longdouble roundings a pair


@pytest.mark.parametrize("kernel", PC.KERNELS)
def test_reference_against_mpmath(kernel):
    c = single_pairs()
    ref, A = PC.REFERENCE[kernel](c)
    for it, t64 in enumerate(c.r_trg):
        t = [mpf(float(x)) for x in t64]
        if kernel in VELOCITY_OF:
            vel = VELOCITY_OF[kernel]
            if vel != "rotlet" and np.array_equal(t64, c.r_src[0]):
                assert not ref[it].any() and not A[it].any()  # masked
                continue
            want = [[mpmath.diff(lambda *p: mp_velocity(vel, c, p)[i], t,
                                 tuple(int(j == k) for k in range(3)))
                     for j in range(3)] for i in range(3)]
        else:
            want = mp_velocity(kernel, c, t)
        want = np.array(want, dtype=object).reshape(ref[it].shape)
        for idx in np.ndindex(ref[it].shape):
            err = abs(to_mp(ref[it][idx]) - want[idx])
            # mpmath.diff is good to about half the working precision
            tol = mpf(float(MP_TOL * A[it][idx])) + abs(want[idx]) * mpf(10) ** -22
            assert err <= tol, (kernel, it, idx, err, tol)


def test_dense_references_against_mpmath():
    pts = PC.fiber_points(1, 4)[0]
    nrm = PC.cloud(73, 4, 1).nrm
    ref, A = R.oseen_tensor(pts, 1.3)
    ref2, A2 = R.stresslet_times_normal(pts, nrm)
    P = [[mpf(float(x)) for x in p] for p in pts]
    N = [[mpf(float(x)) for x in p] for p in nrm]
    for i in range(4):
        for j in range(4):
            # oseen_tensor: block (t, s) = (i, j), d = p_j - p_i
            d = [P[j][k] - P[i][k] for k in range(3)]
            r2 = sum(x * x for x in d)
            y = 0 if r2 == 0 else 1 / mpmath.sqrt(mp_den(r2, PC.REG, PC.EPS, "oseen"))
            # stresslet_times_normal: d = p_i - p_j (enters three times: the sign matters)
            y5 = 0 if i == j else mp_den(r2, PC.REG, PC.EPS, "rotlet") ** mpf(-2.5)
            dn = -sum(d[k] * N[j][k] for k in range(3))
            for a in range(3):
                for b in range(3):
                    want = (y * (a == b) + y ** 3 * d[a] * d[b]) / (8 * mpmath.pi * mpf(1.3))
                    e = 3 * i + a, 3 * j + b
                    assert abs(to_mp(ref[e]) - want) <= mpf(float(MP_TOL * A[e]))
                    want = -3 / (4 * mpmath.pi) * dn * y5 * d[a] * d[b]
                    assert abs(to_mp(ref2[e]) - want) <= mpf(float(MP_TOL * A2[e]))


# ---- gradients against differences of the velocities --------------------------

def _central(field, t, h):
    Gd = np.zeros((len(t), 3, 3), LD)
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        Gd[:, :, j] = (field(t + e)[0] - field(t - e)[0]) / (LD(2) * LD(h))
    return Gd


def _norm(a):
    return np.sqrt((a * a).sum())


@pytest.mark.parametrize("kernel,where", [
    ("stokeslet_grad", "far"), ("stresslet_grad", "far"), ("oseen_grad", "far"),
    ("rotlet_grad", "far"), ("oseen_grad", "regularized"), ("rotlet_grad", "regularized")])
def test_gradient_references_are_derivatives(kernel, where):
    """Central differences with steps h and h/2 (exact in fp64: everything sits
    on a binary grid) miss the gradient by c h^2 and c h^2 / 4."""
    grid = 2.0 ** -30
    c = PC.cloud(81, 5, 6)
    c = PC.replace(c, r_src=np.round(c.r_src / grid) * grid)
    if where == "far":
        u = c.r_trg / np.linalg.norm(c.r_trg, axis=1)[:, None]
        trg, h = np.round(2.5 * u / grid) * grid, 2.0 ** -10
    else:
        # 2e-6 from a source, under eps; the field varies over reg = 5e-3
        trg, h = c.r_src + np.array([2.0 ** -19, -2.0 ** -20, 2.0 ** -21]), 2.0 ** -21
    c = PC.replace(c, r_trg=trg)
    vel = PC.REFERENCE[VELOCITY_OF[kernel]]
    field = lambda p: vel(PC.replace(c, r_trg=p))
    Gref = PC.REFERENCE[kernel](c)[0]
    e1 = _norm(_central(field, trg, h) - Gref)
    e2 = _norm(_central(field, trg, h / 2) - Gref)
    print(f"{kernel} {where}: rel err {float(e1 / _norm(Gref)):.2e} at h, ratio {float(e1 / e2):.4f}")
    assert 3.8 < e1 / e2 < 4.2
    scale = 2.5 if where == "far" else PC.REG
    assert e1 / _norm(Gref) < 20 * (h / scale) ** 2


# ---- the condition sum ---------------------------------------------------------

@pytest.mark.parametrize("kernel", PC.KERNELS)
def test_condition_sum_dominates_and_vanishes_only_when_masked(kernel):
    """Three sources at one point; target 0 sits on them, the others do not."""
    c = PC.cloud(91, 3, 9)
    p = c.r_src[0].copy()
    c.r_src[:] = p
    c.r_trg[0] = p
    ref, A = PC.REFERENCE[kernel](c)
    assert (A >= np.abs(ref)).all()
    if kernel in ("rotlet", "rotlet_grad"):  # no mask: regularized
        assert not A[0].any() if kernel == "rotlet" else A[0].any()
    else:
        assert not A[0].any() and not ref[0].any()
    assert (A[1:] > 0).all()
    for name in ("near", "pair_3x257"):
        ref, A = PC.reference(name, kernel, PC.CASES[name][0])
        assert (A >= np.abs(ref)).all()
