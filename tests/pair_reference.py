"""Extended-precision references of the pair kernels, with the condition sum
and the rounding bound that judge a kernel per target and per component.

Every functor of skellysim_amd/csrc/pair_functors.hpp and the two dense
builders of pair_kernels.hip are restated here from their formulas in
np.longdouble (64-bit mantissa), vectorised over (targets, sources). Each function returns
(ref, A): `ref` is the value, `A` has its shape and is the same expression
with every product replaced by its absolute value and every sum by a sum of
absolute values, prefactor included: the condition sum. |out - ref| is judged
against bound(A, ...), which stays meaningful where a component cancels.
Where A == 0 (every pair of the target masked) the output must be exactly 0.

Conventions are the kernels': d = t - s (the sign of d does not matter where
d enters twice), y = 1/sqrt(den),
    den = r2                                   stokeslet, stresslet (+ grads)
    den = r2 > eps^2 ? r2 : r2 + reg^2         oseen (+ grad), oseen_tensor
    den = r2 < eps^2 ? r2 + reg^2 : r2         rotlet (+ grad), normal-density,
                                               stresslet_times_normal
the r == 0 mask where the functor has one (all but the rotlet pair), gradients
G[t, i, j] = d u_i / d x_j row-major. Branches are chosen from the exact r2
against eps^2, and no pair of a case may lie within a relative 2^-30 of the
threshold (asserted), so neither the kernels' `r2 > eps^2` for the
reference's `r > eps` nor the rounding of eps * eps can matter.

Constants: E_SEED and E_RSQ are measured, profiles/pair_accuracy.md.
"""

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, \
    f"np.longdouble is too narrow to judge fp64 kernels (eps = {np.finfo(LD).eps})"

U = LD(2.0) ** -53  # unit roundoff of fp64
PI = LD("3.14159265358979323846264338327950288")
THRESHOLD_GUARD = LD(2.0) ** -30

# The relative error of the raw v_rsq_f64 seed, |seed * sqrt(x) - 1|: twice the
# maximum that tests/test_gpu_rsq.py measured on MI355X over 2^17 arguments
# (profiles/pair_accuracy.md: 5.1529e-8 = 2^-24.2 for x in [2, 4) 4^k, 3.0350e-8
# for x in [1, 2) 4^k; the sweep samples 2^17 of 2^52 mantissas, hence the
# factor).
E_SEED = LD(2) * LD("5.1529e-8")
# rsq_x2 = y * fma(-(x*y), y, 3) for a seed y = (1 + e) / sqrt(x):
# y (3 - x y^2) = (2 / sqrt(x)) (1 - 1.5 e^2 - 0.5 e^3), and three roundings
# (t = x*y enters q = 3 - t*y, which is ~2, with weight 1/2; q and the product
# with weight 1 each): 1.5 E_SEED^2 + 2.5 u = 1.62e-14 = 146 u, of which the
# sweep reaches 36.5 u (1.5 * 5.15e-8^2 is 35.9 u): one Newton step on this seed
# does not reach the fp64 rounding floor for a single pair.
E_RSQ = LD("1.5") * E_SEED * E_SEED + LD("2.5") * U

# ---- K_ops and P ------------------------------------------------------------
# bound = ((n_src + n_slices) u + K_ops u + P E_RSQ) A, first order.
# (n_src + n_slices) u is the accumulation: one rounding a source in the pair
# loop, one a slice in the reduction. P is the highest power of R = rsq_x2(den)
# in a term of the functor. K_ops counts the rounded fp64 operations on the
# longest path of pair() from the inputs to the accumulator, the accumulating
# fma itself left out (it is the n_src part); an operation whose result enters
# the term with a power p counts p times. Shared pieces:
#   d     1      t - s
#   dot   4      a.d: d, one product, two fmas
#   den   2.5    r2 = dx dx + dy dy + dz dz: d twice (2), three roundings, 5 in
#                all, halved by the square root; 3 where the functor may add
#                reg^2 (one more rounding, and reg * reg's own stays below it)
#   scale 3      M_PI for pi, and the two roundings of the host's
#                1/8/pi/eta or 1/(8 pi eta); the division by ACC_FOLD is exact
#   fin   1      the finish multiply
# Where pair() accumulates twice a source (oseen: y rho, then d c; the
# gradients: an fma and an add, or two fmas), the second accumulation is on the
# path and counts once in K_ops.
K_OPS = {
    # R (d inner + f): dot 4, R^2 1, inner 1, d 1, the inner fma 1 -> 8;
    # 3 den = 7.5; fin, scale
    "stokeslet": 8 + 7.5 + 1 + 3,
    # d coeff: coeff's first term s d^2: d^2 3, product 1, five fmas -> 9;
    # R^2, R^3, R^5 3; -3 R^5 1; coeff product 1; d 1 -> 15; 5 den = 12.5
    "stresslet": 15 + 12.5 + 1 + 3,
    # d (y^3 (d.rho)): y^3 2, dot 4, product 1, d 1, second accumulation 1 -> 9;
    # 3 den = 9
    "oseen": 9 + 9 + 1 + 3,
    # y^3 c: y^3 2, c = fma(d, rho, -(d rho)) 3 -> 5; 3 den = 9
    "rotlet": 5 + 9 + 1 + 3,
    # (d.rho)(d.n) y^5 d: y^5 3, two dots 8, their product 1, times y^5 1, d 1
    # -> 14; 5 den = 15; scale is -3/(4 pi): M_PI and one division, 2
    "normal_density": 14 + 15 + 1 + 2,
    # off-diagonal d_i (B d_j + R^3 f_j) - (R^3 f_i) d_j with
    # B = (f.d) R^3 (-0.75 R^2): dot 4, R^2 1 (twice: in R^3 and in -0.75 R^2),
    # R^3 1, -0.75 R^2 1, A 1, B 1 -> 10; B d_j 2, the add 1, d_i 1, second
    # accumulation 1 -> 15; 5 den = 15
    "stokeslet_grad": 15 + 15 + 1 + 3,
    # diagonal d_i (Bq d_i + R^5 b_i) + A with A = c2 (0.5 R^5),
    # Bq = A (-1.25 R^2): b 4 (sum or d, product, two fmas), c2 = b.d 4 more
    # -> 8; R^5 3, A 1 -> 12; R^2 1, -1.25 R^2 1, Bq 1 -> 15; Bq d 1, the fma 1,
    # d_i 1, second accumulation 1 -> 19; 7 den = 17.5; scale has -3 * scale, 4
    "stresslet_grad": 19 + 17.5 + 1 + 4,
    # q c_i d_j -+ R^3 rho_k with q = (-0.75 R^2) R^3: R^2 twice 2, R^3 1,
    # -0.75 R^2 1, q 1 -> 5; c 3, q c 1, d_j 1, second accumulation 1 -> 11;
    # 5 den = 15
    "rotlet_grad": 11 + 15 + 1 + 3,
    # dense builders, one entry each: no sum, no finish.
    # fr delta_ab + gr d_a d_b: fr 1, gr 2 more, two products 2, d twice 2,
    # the add 1 -> 8; 3 den = 9; factor 1/(8 pi eta): 3
    "oseen_tensor": 8 + 9 + 3,
    # (factor (d.n) y^5) d_a d_b: dot 4, factor product 1, y^5 3, product 1,
    # two products 2, d twice 2 -> 13; 5 den = 15; factor -3/(4 pi): 2
    "stresslet_times_normal": 13 + 15 + 2,
}
P_RSQ = {
    "stokeslet": 3, "stresslet": 5, "oseen": 3, "rotlet": 3, "normal_density": 5,
    "stokeslet_grad": 5, "stresslet_grad": 7, "rotlet_grad": 5,
    "oseen_tensor": 3, "stresslet_times_normal": 5,
}
K_OPS["oseen_grad"], P_RSQ["oseen_grad"] = K_OPS["stokeslet_grad"], P_RSQ["stokeslet_grad"]


def bound(A, n_src, n_slices, kernel):
    """The rounding bound of `kernel` summed over n_src sources in n_slices
    slices, per entry of the condition sum A (longdouble)."""
    c = LD(n_src + n_slices) * U + LD(K_OPS[kernel]) * U + LD(P_RSQ[kernel]) * E_RSQ
    return c * np.asarray(A, LD)


def entry_bound(A, kernel):
    """bound() of a dense builder: each entry is one pair, nothing is summed."""
    return bound(A, 0, 0, kernel)


def excess(out, ref, A):
    """max |out - ref| / (u A) over the entries with A > 0 (0 if none)."""
    err = np.abs(np.asarray(out, LD) - ref)
    ok = A > 0
    return float((err[ok] / (U * A[ok])).max()) if ok.any() else 0.0


# ---- shared pieces -----------------------------------------------------------

BLOCK = 128  # targets per block of the (targets x sources) intermediates


def _ld(a, cols):
    return np.asarray(a, np.float64).reshape(-1, cols).astype(LD)


def _blocked(pair_block, r_trg, shape):
    """pair_block(t) -> (ref, A) over blocks of targets."""
    t = _ld(r_trg, 3)
    ref = np.zeros((len(t),) + shape, LD)
    A = np.zeros((len(t),) + shape, LD)
    for i in range(0, len(t), BLOCK):
        ref[i:i + BLOCK], A[i:i + BLOCK] = pair_block(t[i:i + BLOCK])
    return ref, A


def _sep(t, s):
    """d[t, s, :] = t - s and r2 = |d|^2."""
    d = t[:, None, :] - s[None, :, :]
    return d, (d * d).sum(axis=2)


def _guard(r2, eps):
    eps2 = LD(eps) * LD(eps)
    if eps2 > 0:
        close = np.abs(r2 - eps2) <= THRESHOLD_GUARD * eps2
        assert not close.any(), \
            f"{np.count_nonzero(close)} pairs within 2^-30 of the eps^2 threshold"
    return eps2


def _y(r2, den, mask):
    """1/sqrt(den); 0 at r2 == 0 where the functor masks."""
    with np.errstate(divide="ignore", invalid="ignore"):
        y = LD(1) / np.sqrt(den)
    return np.where(r2 == 0, LD(0), y) if mask else y


def _den_oseen(r2, reg, eps):
    eps2 = _guard(r2, eps)
    return np.where(r2 > eps2, r2, r2 + LD(reg) * LD(reg))


def _den_rotlet(r2, reg, eps):
    eps2 = _guard(r2, eps)
    return np.where(r2 < eps2, r2 + LD(reg) * LD(reg), r2)


def _dot(d, v):
    """(v.d, sum_k |v_k d_k|) for v of shape (sources, 3)."""
    p = d * v[None, :, :]
    return p.sum(axis=2), np.abs(p).sum(axis=2)


# ---- velocity functors ---------------------------------------------------------

def _single_layer(r_src, f, r_trg, eta, den_of):
    s, f = _ld(r_src, 3), _ld(f, 3)
    pf = LD(1) / (LD(8) * PI * LD(eta))

    def block(t):
        d, r2 = _sep(t, s)
        y = _y(r2, den_of(r2), True)
        fd, fd_abs = _dot(d, f)
        y3 = y * y * y
        ref = (y[:, :, None] * f[None] + (y3 * fd)[:, :, None] * d).sum(axis=1)
        A = (y[:, :, None] * np.abs(f)[None] + (y3 * fd_abs)[:, :, None] * np.abs(d)).sum(axis=1)
        return pf * ref, np.abs(pf) * A

    return _blocked(block, r_trg, (3,))


def stokeslet(r_src, f, r_trg, eta):
    """u_i = 1/(8 pi eta) sum_s [ f_i / r + d_i (f.d) / r^3 ], r == 0 dropped."""
    return _single_layer(r_src, f, r_trg, eta, lambda r2: r2)


def oseen_contract(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    """The Stokeslet with y = 1/sqrt(r2 > eps^2 ? r2 : r2 + reg^2), r == 0 dropped."""
    return _single_layer(r_src, rho, r_trg, eta, lambda r2: _den_oseen(r2, reg, eps))


def _dSd(d, S):
    """(d^T S d, sum_kl |d_k S_kl d_l|) for S of shape (sources, 3, 3)."""
    p = d[:, :, :, None] * S[None] * d[:, :, None, :]
    return p.sum(axis=(2, 3)), np.abs(p).sum(axis=(2, 3))


def stresslet(r_src, f9, r_trg, eta):
    """u_i = -3/(8 pi eta) sum_s (d^T S d) d_i / r^5, S_kl = f9[3k + l], r == 0 dropped."""
    s, S = _ld(r_src, 3), _ld(f9, 9).reshape(-1, 3, 3)
    pf = LD(-3) / (LD(8) * PI * LD(eta))

    def block(t):
        d, r2 = _sep(t, s)
        y = _y(r2, r2, True)
        y5 = y ** 5
        C, C_abs = _dSd(d, S)
        ref = ((y5 * C)[:, :, None] * d).sum(axis=1)
        A = ((y5 * C_abs)[:, :, None] * np.abs(d)).sum(axis=1)
        return pf * ref, np.abs(pf) * A

    return _blocked(block, r_trg, (3,))


def _cross(d, rho):
    """c = rho x d, the rotlet's u_x = dz rho_y - dy rho_z, and its condition sum."""
    c = np.empty(d.shape, LD)
    c_abs = np.empty(d.shape, LD)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        a, b = rho[None, :, j] * d[:, :, k], rho[None, :, k] * d[:, :, j]
        c[:, :, i], c_abs[:, :, i] = a - b, np.abs(a) + np.abs(b)
    return c, c_abs


def rotlet(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    """u = 1/(8 pi eta) sum_s (rho x d) y^3, y = 1/sqrt(r2 < eps^2 ? r2 + reg^2 : r2);
    no r == 0 mask."""
    s, rho = _ld(r_src, 3), _ld(rho, 3)
    pf = LD(1) / (LD(8) * PI * LD(eta))

    def block(t):
        d, r2 = _sep(t, s)
        y3 = _y(r2, _den_rotlet(r2, reg, eps), False) ** 3
        c, c_abs = _cross(d, rho)
        return pf * (y3[:, :, None] * c).sum(axis=1), pf * (y3[:, :, None] * c_abs).sum(axis=1)

    return _blocked(block, r_trg, (3,))


def stresslet_normal_density(r_src, normals, rho, r_trg, reg=5e-3, eps=1e-5):
    """out_i = -3/(4 pi) sum_s (d.rho)(d.n) d_i y^5, y as the rotlet's, r == 0 dropped."""
    s, n, rho = _ld(r_src, 3), _ld(normals, 3), _ld(rho, 3)
    pf = LD(-3) / (LD(4) * PI)

    def block(t):
        d, r2 = _sep(t, s)
        y5 = _y(r2, _den_rotlet(r2, reg, eps), True) ** 5
        dn, dn_abs = _dot(d, n)
        dr, dr_abs = _dot(d, rho)
        ref = ((dr * dn * y5)[:, :, None] * d).sum(axis=1)
        A = ((dr_abs * dn_abs * y5)[:, :, None] * np.abs(d)).sum(axis=1)
        return pf * ref, np.abs(pf) * A

    return _blocked(block, r_trg, (3,))


# ---- gradient functors ---------------------------------------------------------

I3 = np.eye(3).astype(LD)


def _single_layer_grad(r_src, f, r_trg, eta, den_of):
    s, f = _ld(r_src, 3), _ld(f, 3)
    pf = LD(1) / (LD(8) * PI * LD(eta))
    offdiag = LD(1) - I3  # d_i f_i - f_i d_i is identically zero

    def block(t):
        d, r2 = _sep(t, s)
        y = _y(r2, den_of(r2), True)
        y3, y5 = y ** 3, y ** 5
        fd, fd_abs = _dot(d, f)
        df = d[:, :, :, None] * f[None, :, None, :]      # d_i f_j
        dd = d[:, :, :, None] * d[:, :, None, :]         # d_i d_j
        ref = (y3[:, :, None, None] * (df - df.transpose(0, 1, 3, 2))
               + (y3 * fd)[:, :, None, None] * I3
               - LD(3) * (y5 * fd)[:, :, None, None] * dd).sum(axis=1)
        A = (y3[:, :, None, None] * (np.abs(df) + np.abs(df).transpose(0, 1, 3, 2)) * offdiag
             + (y3 * fd_abs)[:, :, None, None] * I3
             + LD(3) * (y5 * fd_abs)[:, :, None, None] * np.abs(dd)).sum(axis=1)
        return pf * ref, pf * A

    return _blocked(block, r_trg, (3, 3))


def stokeslet_grad(r_src, f, r_trg, eta):
    """G_ij = 1/(8 pi eta) sum_s [ y^3 (d_i f_j - f_i d_j + (f.d) delta_ij)
    - 3 y^5 (f.d) d_i d_j ], y = 1/r, r == 0 dropped."""
    return _single_layer_grad(r_src, f, r_trg, eta, lambda r2: r2)


def oseen_contract_grad(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    """stokeslet_grad with the oseen y: the derivative inside each branch."""
    return _single_layer_grad(r_src, rho, r_trg, eta, lambda r2: _den_oseen(r2, reg, eps))


def stresslet_grad(r_src, f9, r_trg, eta):
    """G_ij = -3/(8 pi eta) sum_s [ y^5 (d_i b_j + C delta_ij) - 5 y^7 C d_i d_j ],
    C = d^T S d, b_j = (S_jl + S_lj) d_l, y = 1/r, r == 0 dropped."""
    s, S = _ld(r_src, 3), _ld(f9, 9).reshape(-1, 3, 3)
    pf = LD(-3) / (LD(8) * PI * LD(eta))

    def block(t):
        d, r2 = _sep(t, s)
        y = _y(r2, r2, True)
        y5, y7 = y ** 5, y ** 7
        C, C_abs = _dSd(d, S)
        Sd = S[None] * d[:, :, None, :]                  # S_jl d_l
        STd = S.transpose(0, 2, 1)[None] * d[:, :, None, :]  # S_lj d_l
        b = (Sd + STd).sum(axis=3)
        b_abs = (np.abs(Sd) + np.abs(STd)).sum(axis=3)
        dd = d[:, :, :, None] * d[:, :, None, :]
        ref = (y5[:, :, None, None] * d[:, :, :, None] * b[:, :, None, :]
               + (y5 * C)[:, :, None, None] * I3
               - LD(5) * (y7 * C)[:, :, None, None] * dd).sum(axis=1)
        A = (y5[:, :, None, None] * np.abs(d)[:, :, :, None] * b_abs[:, :, None, :]
             + (y5 * C_abs)[:, :, None, None] * I3
             + LD(5) * (y7 * C_abs)[:, :, None, None] * np.abs(dd)).sum(axis=1)
        return pf * ref, np.abs(pf) * A

    return _blocked(block, r_trg, (3, 3))


def rotlet_grad(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    """G_ij = 1/(8 pi eta) sum_s [ y^3 eps_ikj rho_k - 3 y^5 c_i d_j ], c = rho x d,
    y as the rotlet's; no r == 0 mask."""
    s, rho = _ld(r_src, 3), _ld(rho, 3)
    pf = LD(1) / (LD(8) * PI * LD(eta))
    # W[s, i, j] = eps_ikj rho_k
    W = np.zeros((len(s), 3, 3), LD)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        W[:, i, j], W[:, j, i] = -rho[:, k], rho[:, k]   # eps_ikj = -1 for (i, j, k) cyclic

    def block(t):
        d, r2 = _sep(t, s)
        y = _y(r2, _den_rotlet(r2, reg, eps), False)
        y3, y5 = y ** 3, y ** 5
        c, c_abs = _cross(d, rho)
        ref = (y3[:, :, None, None] * W[None]
               - LD(3) * y5[:, :, None, None] * c[:, :, :, None] * d[:, :, None, :]).sum(axis=1)
        A = (y3[:, :, None, None] * np.abs(W)[None]
             + LD(3) * y5[:, :, None, None] * c_abs[:, :, :, None]
             * np.abs(d)[:, :, None, :]).sum(axis=1)
        return pf * ref, pf * A

    return _blocked(block, r_trg, (3, 3))


# ---- dense builders ------------------------------------------------------------

def _blocks_to_matrix(B):
    """(n, n, 3, 3) blocks -> (3n, 3n) with entry (3i + a, 3j + b)."""
    n = B.shape[0]
    return B.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)


def oseen_tensor(pts, eta, reg=5e-3, eps=1e-5):
    """One fiber of oseen_tensor_batched: block (t, s) =
    1/(8 pi eta) (y delta_ab + y^3 d_a d_b), y as oseen_contract's, r == 0 blocks zero."""
    p = _ld(pts, 3)
    pf = LD(1) / (LD(8) * PI * LD(eta))
    d, r2 = _sep(p, p)
    y = _y(r2, _den_oseen(r2, reg, eps), True)
    dd = d[:, :, :, None] * d[:, :, None, :]
    ref = y[:, :, None, None] * I3 + (y ** 3)[:, :, None, None] * dd
    A = y[:, :, None, None] * I3 + (y ** 3)[:, :, None, None] * np.abs(dd)
    return _blocks_to_matrix(pf * ref), _blocks_to_matrix(pf * A)


def oseen_tensor_batched(pts, eta, reg=5e-3, eps=1e-5):
    """(nf, n, 3) -> (nf, 3n, 3n), fiber by fiber."""
    both = [oseen_tensor(p, eta, reg, eps) for p in np.asarray(pts, np.float64)]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def stresslet_times_normal(pts, normals, reg=5e-3, eps=1e-5):
    """Block (i, j) = -3/(4 pi) (d.n_j) y^5 d_a d_b, d = r_i - r_j, y as the
    rotlet's; i == j blocks zero."""
    p, n = _ld(pts, 3), _ld(normals, 3)
    pf = LD(-3) / (LD(4) * PI)
    d, r2 = _sep(p, p)
    y5 = _y(r2, _den_rotlet(r2, reg, eps), False) ** 5
    idx = np.arange(len(p))
    y5[idx, idx] = 0
    dn, dn_abs = _dot(d, n)
    dd = d[:, :, :, None] * d[:, :, None, :]
    ref = (dn * y5)[:, :, None, None] * dd
    A = (dn_abs * y5)[:, :, None, None] * np.abs(dd)
    return _blocks_to_matrix(pf * ref), _blocks_to_matrix(np.abs(pf) * A)
