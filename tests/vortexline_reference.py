"""CPU reference of the device vortex-line tracer: streamline_reference's
stepper with the right-hand side and the stop rule apart (a vortex line follows
the vorticity and stops on the velocity), the vorticity of a source cloud from
the longdouble gradient references of tests/pair_reference.py with its condition
sum, and the shared cases of tests/test_vortexlines_cpu.py and
tests/test_gpu_vortexlines.py.

The law is streamline_reference's with two fields: the stages and the recorded
val are rhs(x) = curl u(x), and step 3 tests |stop(x)| > 1e3 with stop = u."""

import functools

import numpy as np

import pair_reference as P
import streamline_reference as S

LD = P.LD
EPS = S.EPS
DONE, SINGULAR, FULL, GAVE_UP = S.DONE, S.SINGULAR, S.FULL, S.GAVE_UP


def trace(rhs, stop, x0, dt_init=0.1, t_final=1.0, abs_err=1e-10, rel_err=1e-6, max_points=4096):
    """One job, as streamline_reference.trace returns it: val and the stages
    from rhs, the singularity stop from stop (rhs's own value where the two
    are the same function)."""
    s = -1.0 if t_final < 0 else 1.0
    x, t, dt = np.array(x0, float).reshape(3), 0.0, s * abs(dt_init)
    xs, ts, vs, errs, accepted = [], [], [], [], []
    status, tries = DONE, 0

    def done():
        return dict(x=np.array(xs).reshape(-1, 3), t=np.array(ts), val=np.array(vs).reshape(-1, 3),
                    count=len(xs), status=status, errs=np.array(errs), accepted=np.array(accepted))

    while True:
        at_end = not s * (t_final - t) > EPS
        if len(xs) == max_points:
            status = FULL
            return done()
        k1 = rhs(x)
        xs.append(x.copy()), ts.append(t), vs.append(k1.copy())
        if at_end:
            return done()
        if np.linalg.norm(k1 if stop is rhs else stop(x)) > 1e3:
            status = SINGULAR
            return done()
        if s * (t + dt - t_final) > EPS:
            dt = t_final - t
        fails = 0
        while True:
            tries += 1
            if tries > 4 * max_points + 1000 or fails >= 1000 or t + dt == t:
                status = GAVE_UP
                return done()
            x5, d, _ = S.ck_step(rhs, x, dt, k1)
            err = S.error_ratio(x, dt, k1, d, abs_err, rel_err)
            errs.append(err)
            accepted.append(err <= 1.0)
            if not err <= 1.0:
                dt *= S.shrink(err) if err == err else 0.2
                fails += 1
                continue
            t, x = t + dt, x5
            if err < 0.5:
                dt *= S.grow(err)
            break


# ---- the vorticity ----------------------------------------------------------------

def curl(G):
    """(G21 - G12, G02 - G20, G10 - G01) of G (..., 3, 3), G[i][j] = du_i/dx_j."""
    return np.stack([G[..., 2, 1] - G[..., 1, 2], G[..., 0, 2] - G[..., 2, 0],
                     G[..., 1, 0] - G[..., 0, 1]], axis=-1)


def curl_condition(A):
    """The curl's condition sum from the gradient's: A21 + A12, A02 + A20, A10 + A01."""
    return np.stack([A[..., 2, 1] + A[..., 1, 2], A[..., 0, 2] + A[..., 2, 0],
                     A[..., 1, 0] + A[..., 0, 1]], axis=-1)


def background_gradient(background):
    """Gb of u_j = uniform_j + x[components_j] * scale_j: Gb[j][components_j] += scale_j."""
    _, scale, comp = background
    Gb = np.zeros((3, 3))
    for j in range(3):
        Gb[j, int(comp[j])] += float(scale[j])
    return Gb


def background_curl(background):
    """The constant curl of the background, fp64."""
    return curl(background_gradient(background))


# the four sets: (keyword, pair_reference function, its argument order, name in P.K_OPS)
_SETS = (("stokeslet", P.stokeslet_grad, "strength", "stokeslet_grad"),
         ("stresslet", P.stresslet_grad, "strength", "stresslet_grad"),
         ("rotlet", P.rotlet_grad, "density", "rotlet_grad"),
         ("oseen", P.oseen_contract_grad, "density", "oseen_grad"))


def cloud_vorticity(eta, stokeslet=None, stresslet=None, rotlet=None, oseen=None,
                    background=None, bodies=None, reg=5e-3, eps=1e-5):
    """w(x) for x (3,) or (n, 3) -> (omega, A_omega), longdouble arrays of x's
    shape: the curl of the four sets' longdouble gradients plus the background's
    constant curl, and its condition sum (A21 + A12, ... of the four sets plus
    the |Gb| of the background). A point inside a body ((n_b, 10) rows {centre,
    radius, velocity, angular velocity}, the last one deciding) has
    omega = 2 w_b exactly and A_omega = 0. w.sets(x) gives the four sets'
    shares {kernel name: (A_set, n_set)} for pair_reference.bound."""
    given = dict(stokeslet=stokeslet, stresslet=stresslet, rotlet=rotlet, oseen=oseen)

    def per_set(p):
        for key, fn, order, kernel in _SETS:
            if given[key] is None or len(given[key][0]) == 0:
                continue
            r, q = given[key]
            if order == "strength":
                G, A = fn(r, q, p, eta)
            else:
                G, A = fn(r, p, q, eta, reg, eps)
            yield kernel, curl(G), curl_condition(A), len(r)

    def inside(p):
        """Index of the deciding body per point, -1 outside all."""
        which = np.full(len(p), -1)
        if bodies is not None:
            for b, row in enumerate(np.asarray(bodies, float).reshape(-1, 10)):
                which[np.linalg.norm(p - row[None, 0:3], axis=1) < row[3]] = b
        return which

    def w(x):
        p = np.ascontiguousarray(np.asarray(x, float).reshape(-1, 3))
        omega, A = np.zeros(p.shape, LD), np.zeros(p.shape, LD)
        for _, c, a, _ in per_set(p):
            omega += c
            A += a
        if background is not None:
            Gb = background_gradient(background).astype(LD)
            omega += curl(Gb)[None, :]
            A += curl_condition(np.abs(Gb))[None, :]
        which = inside(p)
        if (which >= 0).any():
            rows = np.asarray(bodies, float).reshape(-1, 10)
            omega[which >= 0] = 2.0 * rows[which[which >= 0], 7:10]
            A[which >= 0] = 0
        return omega.reshape(np.shape(x)), A.reshape(np.shape(x))

    def sets(x):
        p = np.ascontiguousarray(np.asarray(x, float).reshape(-1, 3))
        return {kernel: (a, n) for kernel, _, a, n in per_set(p)}

    w.sets = sets
    w.inside = lambda x: inside(np.asarray(x, float).reshape(-1, 3))
    return w


def as_rhs(w):
    """The fp64 right-hand side of a cloud_vorticity."""
    return lambda x: np.asarray(w(x)[0], np.float64)


def val_bound(w, x, background=None):
    """Per point and component, the bound on |val - omega_ref| of the device
    tracer: the sets' pair_reference.bound at 16 slices (the six butterfly
    levels, the waves, the four sets, the curl and the background add) plus
    4 u (|background curl| + A_omega)."""
    _, A = w(x)
    out = np.zeros(np.shape(A), LD)
    for kernel, (a, n) in w.sets(x).items():
        out += P.bound(a, n, 16, kernel).reshape(np.shape(A))
    bg = np.abs(background_curl(background)).astype(LD) if background is not None else LD(0)
    out = out + 4 * P.U * (bg + A)
    out[np.asarray(A) == 0] = 0  # inside a body, or nothing but the background: exact
    return out


# ---- the mixed cloud of the GPU comparison ----------------------------------------

# The cloud, seeds, background and step control are streamline_reference's; the
# viscosity is not. The vorticity of these sources falls off one power of r
# faster than their velocity, so near a source a vortex line needs many small
# steps: at eta = 16 one of the 14 runs fills 256 points with a threshold
# margin under 1e-4. The sources' vorticity is proportional to 1/eta, so a
# larger eta only slows the lines' clock: at eta = 64 all 14 reach t_final
# within 27 points.
ETA = 64.0
T_FINAL, DT_INIT, MAX_POINTS = S.T_FINAL, S.DT_INIT, 128
# 2e-13: the size of pair_reference.bound for these sets per unit of the
# condition sum, 7 E_RSQ + (n + K_ops) u = 1.6e-13 for the 301 Stokeslets.
PERTURBATION = 2e-13
# Seeds of the mixed cloud that break precondition (a) or (b) under this
# reference: {seed index: which condition}.
DROPPED = {}


def mixed_fields():
    """(w, u): the cloud_vorticity and the oracle velocity of the mixed cloud."""
    import oracle
    sets = S.mixed_sets()
    return cloud_vorticity(ETA, **sets), S.cloud_field(oracle, ETA, **sets)


def _mixed_runs(rhs, stop):
    seeds = S.mixed_cloud()["seeds"]
    return [(i, tf, trace(rhs, stop, seeds[i], DT_INIT, tf, max_points=MAX_POINTS))
            for tf in (T_FINAL, -T_FINAL) for i in range(len(seeds))]


@functools.lru_cache(maxsize=None)
def mixed_reference():
    """The 14 reference runs of the mixed cloud: [(seed, t_final, run)], jobs
    in the tracer's order (all seeds forward, then all backward)."""
    w, u = mixed_fields()
    return _mixed_runs(as_rhs(w), u)


@functools.lru_cache(maxsize=None)
def mixed_perturbed(amplitude=PERTURBATION):
    """The same runs with amplitude * A_omega * xi added to every vorticity
    component, xi uniform in [-1, 1] from default_rng(101), drawn per evaluation
    in call order: the runs' sensitivity to errors of the rounding bound's size."""
    w, u = mixed_fields()
    rng = np.random.default_rng(101)

    def rhs(x):
        omega, A = w(x)
        return np.asarray(omega + LD(amplitude) * A * rng.uniform(-1, 1, np.shape(x)), np.float64)
    return _mixed_runs(rhs, u)


def kept_seeds():
    return [i for i in range(len(S.mixed_cloud()["seeds"])) if i not in DROPPED]


# ---- a large vorticity beside a moderate velocity ----------------------------------

# One Stokeslet of unit force at the origin and a seed 1e-3 away from it, at
# eta = 1: |u| = O(1 / (8 pi r)) = O(1e2) and |omega| = |f x d| / (4 pi r^3) =
# O(1e5). The vortex line is a circle about the force's axis at constant
# |omega| and |u|, so a tracer that stopped on the field it integrates would
# stop at the seed, and one that stops on the velocity runs to t_final.
# t_final: the circle has a radius of 8e-4 and is run at 8e7 rad per unit time,
# so at 1e-6 the step control fills the 128 points (status 2) before the end;
# 3e-7 is the largest of the half decades 1e-6, 3e-7, 1e-7 at which the
# reference finishes (115 points).
NEAR = dict(stokeslet=(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]])),
            seed=np.array([0.6e-3, 0.8e-3, 0.0]), eta=1.0, dt_init=0.1, t_final=3e-7)


def near_fields():
    import oracle
    return (cloud_vorticity(NEAR["eta"], stokeslet=NEAR["stokeslet"]),
            S.cloud_field(oracle, NEAR["eta"], stokeslet=NEAR["stokeslet"]))


@functools.lru_cache(maxsize=None)
def near_reference():
    w, u = near_fields()
    return trace(as_rhs(w), u, NEAR["seed"], NEAR["dt_init"], NEAR["t_final"],
                 max_points=MAX_POINTS)
