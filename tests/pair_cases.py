"""The inputs of the per-target accuracy tests, shared by the CPU tests of the
references (test_pair_reference.py) and the GPU tests of the kernels
(test_gpu_pair_accuracy.py), and the references by kernel name.

A case is a Case: clouds, strengths and the scalar parameters of every kernel;
each kernel reads what it needs (f3 is the force, density or torque, f9 the
stresslet tensor, nrm the normals of the normal-density functor)."""

from dataclasses import dataclass, replace

import numpy as np

import pair_reference as R

REG, EPS = 5e-3, 1e-5  # the kernels' defaults


@dataclass
class Case:
    r_src: np.ndarray
    r_trg: np.ndarray
    f3: np.ndarray
    f9: np.ndarray
    nrm: np.ndarray
    eta: float = 1.3
    reg: float = REG
    eps: float = EPS

    @property
    def n_src(self):
        return len(self.r_src)


def cloud(seed, n_src, n_trg, **kw):
    rng = np.random.default_rng(seed)
    return Case(r_src=rng.uniform(-1, 1, (n_src, 3)), r_trg=rng.uniform(-1, 1, (n_trg, 3)),
                f3=rng.uniform(-1, 1, (n_src, 3)), f9=rng.uniform(-1, 1, (n_src, 9)),
                nrm=rng.uniform(-1, 1, (n_src, 3)), **kw)


def _directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def near_cloud(seed=11, n_src=300, n_near=129, n_far=20, **kw):
    """Targets are the first n_near sources: every third exact, every third
    displaced by 3e-6 (under eps), every third by 1e-4 (over it); n_far plain
    targets behind them."""
    c = cloud(seed, n_src, n_far, **kw)
    rng = np.random.default_rng(seed + 1)
    step = np.array([0.0, 3e-6, 1e-4])[np.arange(n_near) % 3]
    near = c.r_src[:n_near] + step[:, None] * _directions(rng, n_near)
    return replace(c, r_trg=np.concatenate([near, c.r_trg]))


def threshold_cloud(seed=21, n_src=40, reg=REG, eps=EPS):
    """Target 4 k + m sits at eps (1 + o_m) from source k,
    o = (-2^-10, -2^-20, 2^-20, 2^-10)."""
    c = cloud(seed, n_src, 1, reg=reg, eps=eps)
    rng = np.random.default_rng(seed + 1)
    off = np.array([-2.0 ** -10, -2.0 ** -20, 2.0 ** -20, 2.0 ** -10])
    dist = eps * (1.0 + np.tile(off, n_src))
    trg = np.repeat(c.r_src, 4, axis=0) + dist[:, None] * _directions(rng, 4 * n_src)
    return replace(c, r_trg=trg)


def self_cloud(seed=31, n=70, **kw):
    """One point set as sources and targets (every target coincides with a
    source), three of the points duplicated."""
    c = cloud(seed, n, 1, **kw)
    c.r_src[40:43] = c.r_src[3:6]
    return replace(c, r_trg=c.r_src)


def scale_cloud(seed=41, n_src=131, n_trg=513, n_near=20):
    """The 131-source case with its first n_near targets 3e-6 from a source."""
    c = cloud(seed, n_src, n_trg)
    rng = np.random.default_rng(seed + 1)
    c.r_trg[:n_near] = c.r_src[:n_near] + 3e-6 * _directions(rng, n_near)
    return c


def scaled(c, s, with_params):
    """The cloud times s (a power of two: exact); reg and eps with it or not."""
    return replace(c, r_src=c.r_src * s, r_trg=c.r_trg * s,
                   reg=c.reg * s if with_params else c.reg,
                   eps=c.eps * s if with_params else c.eps)


def translated(c, shift=(1000.0, -1000.0, 500.0)):
    shift = np.asarray(shift)
    return replace(c, r_src=c.r_src + shift, r_trg=c.r_trg + shift)


# (ref, A) of a case, by kernel
REFERENCE = {
    "stokeslet": lambda c: R.stokeslet(c.r_src, c.f3, c.r_trg, c.eta),
    "stresslet": lambda c: R.stresslet(c.r_src, c.f9, c.r_trg, c.eta),
    "oseen": lambda c: R.oseen_contract(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
    "rotlet": lambda c: R.rotlet(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
    "normal_density": lambda c: R.stresslet_normal_density(c.r_src, c.nrm, c.f3, c.r_trg,
                                                           c.reg, c.eps),
    "stokeslet_grad": lambda c: R.stokeslet_grad(c.r_src, c.f3, c.r_trg, c.eta),
    "stresslet_grad": lambda c: R.stresslet_grad(c.r_src, c.f9, c.r_trg, c.eta),
    "oseen_grad": lambda c: R.oseen_contract_grad(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
    "rotlet_grad": lambda c: R.rotlet_grad(c.r_src, c.r_trg, c.f3, c.eta, c.reg, c.eps),
}
KERNELS = list(REFERENCE)
# the kernels that read reg and eps
REGULARIZED = ["oseen", "rotlet", "normal_density", "oseen_grad", "rotlet_grad"]
# ... and of those, the ones whose reg = 0 reference is finite at r = 0 (masked)
MASKED_REGULARIZED = ["oseen", "normal_density", "oseen_grad"]

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


def fiber_points(nf, n, seed=51):
    """(nf, n, 3) fiber points; in fibers of 3 or more points, points 0 and 1
    of fiber 0 are 4e-6 apart and point 2 of the last fiber repeats point 0."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (nf, n, 3))
    if n >= 3:
        pts[0, 1] = pts[0, 0] + 4e-6 * _directions(rng, 1)[0]
        pts[-1, 2] = pts[-1, 0]
    return pts


def surface_points(n, seed=60):
    """A Case whose r_src and nrm feed stresslet_times_normal; with 3 or more
    points, point 1 is 3.7e-6 from point 0 and point 2 repeats it."""
    c = cloud(seed + n, n, 1)
    if n >= 3:
        c.r_src[1] = c.r_src[0] + np.array([3e-6, -2e-6, 1e-6])
        c.r_src[2] = c.r_src[0]
    return c


# The named cases both test files walk: name -> (case, forced slice counts).
def _named_cases():
    out = {}
    for n in (1, 2, 3, 5):
        out[f"pair_{n}x257"] = (cloud(100 + n, n, 257), (1,))
    for n_trg in (1, 513, 1025):
        out[f"driver_131x{n_trg}"] = (cloud(200 + n_trg, 131, n_trg), (1, 3))
    out["driver_1300x1100"] = (cloud(300, 1300, 1100), (1,))
    out["near"] = (near_cloud(), (1, 3))
    base = scale_cloud()
    out["scale_1"] = (base, (1,))
    for tag, s in (("down", 2.0 ** -10), ("up", 2.0 ** 10)):
        out[f"scale_{tag}"] = (scaled(base, s, False), (1,))
        out[f"scale_{tag}_params"] = (scaled(base, s, True), (1,))
    out["translated"] = (translated(base), (1,))
    return out


CASES = _named_cases()

# Regularized kernels only: name -> (case, slice counts).
THRESHOLD_CASES = {
    "threshold_default": (threshold_cloud(), (1,)),
    "threshold_reg2e-3_eps3e-5": (threshold_cloud(seed=22, reg=2e-3, eps=3e-5), (1,)),
    "near_reg2e-3_eps3e-5": (near_cloud(seed=12, reg=2e-3, eps=3e-5), (1,)),
}
# reg = 0 with coincident pairs, for MASKED_REGULARIZED
REG0_CASES = {
    "self_reg0": (self_cloud(reg=0.0), (1, 3)),
}
