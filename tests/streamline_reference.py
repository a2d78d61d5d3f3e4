"""CPU reference of the device streamline tracer: a numpy restatement of its
stepper (Cash-Karp 5(4) under Boost.Odeint's controlled_runge_kutta law, as
DESIGN.md "Streamlines on the device" states it) over the oracle's velocity
kernels, and the shared cases of tests/test_streamlines_cpu.py and
tests/test_gpu_streamlines.py. trace() records every try's err, so that the
tests can tell how far every accept/reject decision was from its threshold.

The law, with s = sign(t_final):
 1. loop while s (t_final - t) > DBL_EPSILON;
 2. record (x, t, u(x));
 3. |u(x)| > 1e3: stop, status 1 (the point stays recorded);
 4. s (t + dt - t_final) > DBL_EPSILON: dt = t_final - t;
 5. try the step, err = max_i |x5_i - x4_i| / (abs + rel (|x_i| + |dt| |u_i(x)|));
 6. err > 1: dt *= max(0.9 err^(-1/3), 0.2), retry;
 7. else t += dt, x = x5, and if err < 0.5: dt *= 0.9 max(5^-5, err)^(-1/5);
 8. after the loop, record the end point.
1000 failed tries of one step, t + dt == t, or more than 4 max_points + 1000
tries give status 3; a full buffer status 2 with count == max_points."""

import functools
from fractions import Fraction as Fr

import numpy as np

EPS = np.finfo(float).eps
DONE, SINGULAR, FULL, GAVE_UP = 0, 1, 2, 3

# Cash-Karp: nodes, stage rows, 5th- and 4th-order weights
C = [Fr(0), Fr(1, 5), Fr(3, 10), Fr(3, 5), Fr(1), Fr(7, 8)]
A = [[],
     [Fr(1, 5)],
     [Fr(3, 40), Fr(9, 40)],
     [Fr(3, 10), Fr(-9, 10), Fr(6, 5)],
     [Fr(-11, 54), Fr(5, 2), Fr(-70, 27), Fr(35, 27)],
     [Fr(1631, 55296), Fr(175, 512), Fr(575, 13824), Fr(44275, 110592), Fr(253, 4096)]]
B5 = [Fr(37, 378), Fr(0), Fr(250, 621), Fr(125, 594), Fr(0), Fr(512, 1771)]
B4 = [Fr(2825, 27648), Fr(0), Fr(18575, 48384), Fr(13525, 55296), Fr(277, 14336), Fr(1, 4)]
_A = [[float(a) for a in row] for row in A]
_B5 = np.array([float(b) for b in B5])
_DB = np.array([float(b5 - b4) for b5, b4 in zip(B5, B4)])


def ck_step(f, x, dt, k1):
    """One Cash-Karp step from x with k1 = f(x): (x5, x5 - x4, stages (6, 3))."""
    k = np.zeros((6, 3))
    k[0] = k1
    for i in range(1, 6):
        k[i] = f(x + dt * (np.array(_A[i]) @ k[:i]))
    return x + dt * (_B5 @ k), dt * (_DB @ k), k


def error_ratio(x, dt, k1, d, abs_err, rel_err):
    return float(np.max(np.abs(d) / (abs_err + rel_err * (np.abs(x) + abs(dt) * np.abs(k1)))))


def shrink(err):
    """Factor of dt after a rejected try."""
    return max(0.9 * err ** (-1.0 / 3.0), 0.2)


def grow(err):
    """Factor of dt after a step accepted with err < 0.5."""
    return 0.9 * max(5.0 ** -5, err) ** (-1.0 / 5.0)


def trace(f, x0, dt_init=0.1, t_final=1.0, abs_err=1e-10, rel_err=1e-6, max_points=4096):
    """One job: dict(x (count, 3), t, val, count, status, errs (every try's
    err, in order), accepted (per try))."""
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
        k1 = f(x)
        xs.append(x.copy()), ts.append(t), vs.append(k1.copy())
        if at_end:
            return done()
        if np.linalg.norm(k1) > 1e3:
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
            x5, d, _ = ck_step(f, x, dt, k1)
            err = error_ratio(x, dt, k1, d, abs_err, rel_err)
            errs.append(err)
            accepted.append(err <= 1.0)
            if not err <= 1.0:
                dt *= shrink(err) if err == err else 0.2
                fails += 1
                continue
            t, x = t + dt, x5
            if err < 0.5:
                dt *= grow(err)
            break


# ---- fields -----------------------------------------------------------------------

def cloud_field(oracle, eta, stokeslet=None, stresslet=None, rotlet=None, oseen=None,
                background=None, bodies=None):
    """f(x) for x (3,) or (n, 3): the oracle's velocity of the four sets
    ((r_src, strength) or None) plus the background (uniform, scale_factor,
    components) with the rigid motion inside bodies ((n_b, 10) rows {centre,
    radius, velocity, angular velocity}): what the tracer integrates."""
    def f(x):
        p = np.ascontiguousarray(np.asarray(x, float).reshape(-1, 3))
        u = np.zeros_like(p)
        if stokeslet is not None:
            u += oracle.stokeslet(stokeslet[0], stokeslet[1], p, eta)
        if stresslet is not None:
            u += oracle.stresslet(stresslet[0], stresslet[1], p, eta)
        if rotlet is not None:
            u += oracle.rotlet(rotlet[0], p, rotlet[1], eta)
        if oseen is not None:
            u += oracle.oseen_contract(oseen[0], p, oseen[1], eta)
        if background is not None:
            uniform, scale, comp = background
            u += np.asarray(uniform)[None, :] + p[:, list(comp)] * np.asarray(scale)[None, :]
        if bodies is not None:
            for b in np.asarray(bodies, float).reshape(-1, 10):
                dx = p - b[None, 0:3]
                inside = np.linalg.norm(dx, axis=1) < b[3]
                u[inside] = b[None, 4:7] + np.cross(b[None, 7:10], dx[inside])
        return u.reshape(np.shape(x))
    return f


# ---- the mixed cloud of the GPU comparison ----------------------------------------

# The viscosity is this file's choice. The cloud's stresslets have strengths of
# order 1 like its Stokeslets, and a stresslet's flow is radial (u ~ d / r^3):
# lines run into the sources. At eta = 1 all 14 reference runs end in such a
# 1/r^2 singularity before |t| = 1 (status 1), where the end point is as
# sensitive to rounding as anything can be (precondition (b) fails by up to
# two decades), at eta = 8 six of them do. The sources' velocity is
# proportional to 1/eta, so a larger eta only slows their clock: at eta = 16
# twelve runs reach t_final and two still end in a singularity (status 1 stays
# covered), and all 14 keep both preconditions.
ETA = 16.0
T_FINAL, DT_INIT = 1.0, 0.1
BACKGROUND = ((0.1, -0.05, 0.02), (0.3, -0.2, 0.1), (1, 2, 0))
# Seeds of the mixed cloud that break precondition (a) or (b) under this
# reference (tests/test_streamlines_cpu.py checks the others, and that these
# are the only ones): {seed index: which condition}.
DROPPED = {}


@functools.lru_cache(maxsize=None)
def mixed_cloud():
    """default_rng(100), uniform in [-1, 1], in this order: 301 Stokeslet
    positions and forces (one full pass of a 256-thread group and a
    remainder), 5 rotlet centres and torques (less than one pass), 7 seeds,
    then 97 stresslet sources and 3 Oseen sources."""
    rng = np.random.default_rng(100)
    u = lambda *shape: rng.uniform(-1, 1, shape)
    c = dict(stokeslet=(u(301, 3), u(301, 3)), rotlet=(u(5, 3), u(5, 3)))
    c["seeds"] = u(7, 3)
    c["stresslet"] = (u(97, 3), u(97, 9))
    c["oseen"] = (u(3, 3), u(3, 3))
    c["background"] = BACKGROUND
    return c


def mixed_sets(c=None):
    c = c or mixed_cloud()
    return {k: c[k] for k in ("stokeslet", "stresslet", "rotlet", "oseen", "background")}


@functools.lru_cache(maxsize=None)
def mixed_reference():
    """The 14 reference runs of the mixed cloud: [(seed, t_final, run)], jobs
    in the tracer's order (all seeds forward, then all backward)."""
    import oracle
    c = mixed_cloud()
    f = cloud_field(oracle, ETA, **mixed_sets(c))
    return [(i, tf, trace(f, c["seeds"][i], DT_INIT, tf))
            for tf in (T_FINAL, -T_FINAL) for i in range(len(c["seeds"]))]


@functools.lru_cache(maxsize=None)
def mixed_perturbed():
    """The same runs with every velocity multiplied by 1 + 1e-13 xi, xi uniform
    in [-1, 1]: the sensitivity of the runs to rounding-size changes of u."""
    import oracle
    c = mixed_cloud()
    f = cloud_field(oracle, ETA, **mixed_sets(c))
    rng = np.random.default_rng(101)
    g = lambda x: f(x) * (1.0 + 1e-13 * rng.uniform(-1, 1, np.shape(x)))
    return [(i, tf, trace(g, c["seeds"][i], DT_INIT, tf))
            for tf in (T_FINAL, -T_FINAL) for i in range(len(c["seeds"]))]


def threshold_margin(run):
    """Smallest relative distance of a try's err from 1 and from 0.5."""
    e = run["errs"]
    return float(min(np.min(np.abs(e - 1.0)), np.min(np.abs(e - 0.5) / 0.5))) if len(e) else 1.0


def kept_seeds():
    return [i for i in range(len(mixed_cloud()["seeds"])) if i not in DROPPED]
