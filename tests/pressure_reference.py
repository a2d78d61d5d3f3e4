"""Extended-precision references of the pressure functors (StokesletPressure,
StressletPressure of skellysim_amd/csrc/pair_functors.hpp), in the manner of
tests/pair_reference.py and with its conventions: np.longdouble, d = t - s,
y = 1/sqrt(den), the r == 0 mask, (ref, A) with A the condition sum (every
product replaced by its absolute value, every sum by a sum of absolute values,
prefactor included), and the same bound

    ((n_src + n_slices) u + K_ops u + P E_RSQ) A.

    stokeslet   p = 1/(4 pi) sum_s (f.d) y^3                  den = r2
    oseen       the same with den = r2 > eps^2 ? r2 : r2 + reg^2
    stresslet   p = 1/(4 pi) sum_s [ tr(S) y^3 - 3 C y^5 ]    den = r2,
                S_kl = f9[3k + l], C = d^T S d
                A = 1/(4 pi) sum_s [ (|S_xx| + |S_yy| + |S_zz|) y^3 + 3 C_abs y^5 ]

No pressure depends on eta. E_SEED and E_RSQ are pair_reference's (measured,
profiles/pair_accuracy.md); K_ops and P follow the rule written there."""

import numpy as np

import pair_reference as R
from pair_reference import LD, PI, U, E_SEED, E_RSQ  # noqa: F401

K_OPS = {
    # fma(fd, R^3, acc) with R^3 = (R R) R: dot 4 (d, one product, two fmas),
    # R^2 1, R^3 1 -> 6; den may add reg^2: 3, times P = 3 -> 9; fin 1; scale
    # 1/(4 pi): M_PI and one division (4 * M_PI is exact), 2
    "stokeslet_pressure": 6 + 9 + 1 + 2,
    # fma(R^3, q, acc), q = fma(-0.75 R^2, C, tr): C's first term s d^2: d^2 3,
    # product 1, five fmas -> 9 (as the stresslet's coeff); R^2 1, twice (it is
    # in R^3 and in -0.75 R^2) 2; R^3 1; -0.75 R^2 1; the fma of q 1 -> 14 (the
    # tr path, two adds and that fma, is shorter); 5 den = 12.5; fin 1; scale 2
    "stresslet_pressure": 14 + 12.5 + 1 + 2,
}
K_OPS["oseen_pressure"] = K_OPS["stokeslet_pressure"]
# the highest power of R = rsq_x2(den) in a term: y^3, and y^5 in 3 C y^5
P_RSQ = {"stokeslet_pressure": 3, "oseen_pressure": 3, "stresslet_pressure": 5}


def bound(A, n_src, n_slices, kernel):
    """pair_reference.bound with the pressure functors' constants."""
    c = LD(n_src + n_slices) * U + LD(K_OPS[kernel]) * U + LD(P_RSQ[kernel]) * E_RSQ
    return c * np.asarray(A, LD)


def _single_layer_pressure(r_src, f, r_trg, den_of):
    s, f = R._ld(r_src, 3), R._ld(f, 3)
    pf = LD(1) / (LD(4) * PI)

    def block(t):
        d, r2 = R._sep(t, s)
        y3 = R._y(r2, den_of(r2), True) ** 3
        fd, fd_abs = R._dot(d, f)
        return pf * (y3 * fd).sum(axis=1), pf * (y3 * fd_abs).sum(axis=1)

    return R._blocked(block, r_trg, ())


def stokeslet_pressure(r_src, f, r_trg):
    """p = 1/(4 pi) sum_s (f.d) / r^3, r == 0 dropped."""
    return _single_layer_pressure(r_src, f, r_trg, lambda r2: r2)


def oseen_contract_pressure(r_src, r_trg, rho, reg=5e-3, eps=1e-5):
    """The Stokeslet's with y = 1/sqrt(r2 > eps^2 ? r2 : r2 + reg^2), r == 0 dropped."""
    return _single_layer_pressure(r_src, rho, r_trg, lambda r2: R._den_oseen(r2, reg, eps))


def stresslet_pressure(r_src, f9, r_trg):
    """p = 1/(4 pi) sum_s [ tr(S) / r^3 - 3 (d^T S d) / r^5 ], r == 0 dropped."""
    s, S = R._ld(r_src, 3), R._ld(f9, 9).reshape(-1, 3, 3)
    pf = LD(1) / (LD(4) * PI)
    tr = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]
    tr_abs = np.abs(S[:, 0, 0]) + np.abs(S[:, 1, 1]) + np.abs(S[:, 2, 2])

    def block(t):
        d, r2 = R._sep(t, s)
        y = R._y(r2, r2, True)
        y3, y5 = y ** 3, y ** 5
        C, C_abs = R._dSd(d, S)
        ref = (y3 * tr[None, :] - LD(3) * y5 * C).sum(axis=1)
        A = (y3 * tr_abs[None, :] + LD(3) * y5 * C_abs).sum(axis=1)
        return pf * ref, pf * A

    return R._blocked(block, r_trg, ())


# (ref, A) of a pair_cases.Case, by kernel
REFERENCE = {
    "stokeslet_pressure": lambda c: stokeslet_pressure(c.r_src, c.f3, c.r_trg),
    "stresslet_pressure": lambda c: stresslet_pressure(c.r_src, c.f9, c.r_trg),
    "oseen_pressure": lambda c: oseen_contract_pressure(c.r_src, c.r_trg, c.f3, c.reg, c.eps),
}
KERNELS = list(REFERENCE)

_cache = {}


def reference(name, kernel, case):
    """REFERENCE[kernel](case), computed once per (case name, kernel); the
    arrays are read-only."""
    key = (name, kernel)
    if key not in _cache:
        ref, A = REFERENCE[kernel](case)
        ref.setflags(write=False)
        A.setflags(write=False)
        _cache[key] = (ref, A)
    return _cache[key]
