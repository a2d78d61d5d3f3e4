"""CPU tests of the velocity-gradient layers above the kernels: the listener's
velocity_gradient_field and its two protocol extensions, and the sources'
flow_grad. The compute backend is a small numpy class built from the closed
forms below (d = t - s, y = 1/sqrt(den), prefactor 1/(8 pi eta)):

  Stokeslet / regularized Oseen   den = r^2, or r^2 > eps^2 ? r^2 : r^2 + reg^2
      u_i  = y f_i + y^3 (f.d) d_i                      (r^2 == 0 dropped)
      G_ij = y^3 (d_i f_j - f_i d_j + (f.d) delta_ij) - 3 y^5 (f.d) d_i d_j
  Stresslet   S_kl = f[3k+l], C = d_k S_kl d_l, b_j = (S_jl + S_lj) d_l
      u_i  = -3 y^5 C d_i                               (r^2 == 0 dropped)
      G_ij = -3 [ y^5 (d_i b_j + C delta_ij) - 5 y^7 C d_i d_j ]
  Rotlet      den = r^2 < eps^2 ? r^2 + reg^2 : r^2,  c = rho x d
      u_i  = y^3 c_i
      G_ij = y^3 eps_ikj rho_k - 3 y^5 c_i d_j

tests/test_gpu_gradient.py imports the same closed forms as its reference."""

import io
import os
import struct

import msgpack
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

CHUNK = 128  # targets per block of the (targets x sources) intermediates
EPS = np.zeros((3, 3, 3))
EPS[0, 1, 2] = EPS[1, 2, 0] = EPS[2, 0, 1] = 1.0
EPS[0, 2, 1] = EPS[2, 1, 0] = EPS[1, 0, 2] = -1.0
I3 = np.eye(3)


def _chunked(fn, r_trg, shape):
    r_trg = np.asarray(r_trg, float).reshape(-1, 3)
    out = np.zeros((len(r_trg),) + shape)
    for i in range(0, len(r_trg), CHUNK):
        out[i:i + CHUNK] = fn(r_trg[i:i + CHUNK])
    return out


def _sl_terms(r_src, f, t, reg, eps):
    d = t[:, None, :] - r_src[None, :, :]
    r2 = np.einsum("tsk,tsk->ts", d, d)
    den = np.where(r2 > eps * eps, r2, r2 + reg * reg)
    with np.errstate(divide="ignore"):
        y = np.where(r2 == 0.0, 0.0, 1.0 / np.sqrt(den))
    fd = np.einsum("sk,tsk->ts", f, d)
    return d, y, fd


def np_stokeslet(r_src, f, r_trg, eta, reg=0.0, eps=0.0):
    r_src, f = np.asarray(r_src, float), np.asarray(f, float)

    def block(t):
        d, y, fd = _sl_terms(r_src, f, t, reg, eps)
        return np.einsum("ts,si->ti", y, f) + np.einsum("ts,tsi->ti", y ** 3 * fd, d)

    return _chunked(block, r_trg, (3,)) / (8 * np.pi * eta)


def np_stokeslet_grad(r_src, f, r_trg, eta, reg=0.0, eps=0.0):
    r_src, f = np.asarray(r_src, float), np.asarray(f, float)

    def block(t):
        d, y, fd = _sl_terms(r_src, f, t, reg, eps)
        y3 = y ** 3
        G = np.einsum("ts,tsi,sj->tij", y3, d, f) - np.einsum("ts,si,tsj->tij", y3, f, d)
        G += np.einsum("ts,ij->tij", y3 * fd, I3)
        G -= 3.0 * np.einsum("ts,tsi,tsj->tij", y ** 5 * fd, d, d)
        return G

    return _chunked(block, r_trg, (3, 3)) / (8 * np.pi * eta)


def _dl_terms(r_src, f9, t):
    S = f9.reshape(-1, 3, 3)
    d = t[:, None, :] - r_src[None, :, :]
    r2 = np.einsum("tsk,tsk->ts", d, d)
    with np.errstate(divide="ignore"):
        y = np.where(r2 == 0.0, 0.0, 1.0 / np.sqrt(r2))
    C = np.einsum("tsk,skl,tsl->ts", d, S, d)
    b = np.einsum("sjl,tsl->tsj", S + S.transpose(0, 2, 1), d)
    return d, y, C, b


def np_stresslet(r_src, f9, r_trg, eta):
    r_src, f9 = np.asarray(r_src, float), np.asarray(f9, float)

    def block(t):
        d, y, C, _ = _dl_terms(r_src, f9, t)
        return -3.0 * np.einsum("ts,tsi->ti", y ** 5 * C, d)

    return _chunked(block, r_trg, (3,)) / (8 * np.pi * eta)


def np_stresslet_grad(r_src, f9, r_trg, eta):
    r_src, f9 = np.asarray(r_src, float), np.asarray(f9, float)

    def block(t):
        d, y, C, b = _dl_terms(r_src, f9, t)
        y5 = y ** 5
        G = np.einsum("ts,tsi,tsj->tij", y5, d, b) + np.einsum("ts,ij->tij", y5 * C, I3)
        G -= 5.0 * np.einsum("ts,tsi,tsj->tij", y ** 7 * C, d, d)
        return -3.0 * G

    return _chunked(block, r_trg, (3, 3)) / (8 * np.pi * eta)


def _rot_terms(r_src, rho, t, reg, eps):
    d = t[:, None, :] - r_src[None, :, :]
    r2 = np.einsum("tsk,tsk->ts", d, d)
    den = np.where(r2 < eps * eps, r2 + reg * reg, r2)
    y = 1.0 / np.sqrt(den)
    c = np.cross(np.broadcast_to(rho[None, :, :], d.shape), d)
    return d, y, c


def np_rotlet(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    r_src, rho = np.asarray(r_src, float), np.asarray(rho, float)

    def block(t):
        d, y, c = _rot_terms(r_src, rho, t, reg, eps)
        return np.einsum("ts,tsi->ti", y ** 3, c)

    return _chunked(block, r_trg, (3,)) / (8 * np.pi * eta)


def np_rotlet_grad(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    r_src, rho = np.asarray(r_src, float), np.asarray(rho, float)

    def block(t):
        d, y, c = _rot_terms(r_src, rho, t, reg, eps)
        G = np.einsum("ts,ikj,sk->tij", y ** 3, EPS, rho)
        G -= 3.0 * np.einsum("ts,tsi,tsj->tij", y ** 5, c, d)
        return G

    return _chunked(block, r_trg, (3, 3)) / (8 * np.pi * eta)


def np_oseen(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    return np_stokeslet(r_src, rho, r_trg, eta, reg, eps)


def np_oseen_grad(r_src, r_trg, rho, eta, reg=5e-3, eps=1e-5):
    return np_stokeslet_grad(r_src, rho, r_trg, eta, reg, eps)


def curl(G):
    return np.stack([G[..., 2, 1] - G[..., 1, 2], G[..., 0, 2] - G[..., 2, 0],
                     G[..., 1, 0] - G[..., 0, 1]], axis=-1)


def central_difference(field, pts, h=1e-5):
    """G[t, i, j] from 6 probes a point of field: (n, 3) -> (n, 3)."""
    pts = np.asarray(pts, float).reshape(-1, 3)
    G = np.zeros((len(pts), 3, 3))
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        G[:, :, j] = (field(pts + e) - field(pts - e)) / (2 * h)
    return G


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


class NumpyVelocityBackend:
    """The velocity methods of the system_fd.HipBackend contract only."""

    def stokeslet(self, r_src, f_src, r_trg, eta):
        return np_stokeslet(r_src, f_src, r_trg, eta)

    def stresslet_normal_density(self, r_src, normals, density, r_trg, eta):
        f_dl = 2.0 * eta * np.einsum("ni,nj->nij", normals, density).reshape(-1, 9)
        return np_stresslet(r_src, f_dl, r_trg, eta)

    def rotlet(self, centers, torques, r_trg, eta):
        return np_rotlet(centers, r_trg, torques, eta)

    def oseen_contract(self, r_src, r_trg, density, eta):
        return np_oseen(r_src, r_trg, density, eta)


class NumpyBackend(NumpyVelocityBackend):
    """... plus the four gradient methods."""

    def stokeslet_grad(self, r_src, f_src, r_trg, eta):
        return np_stokeslet_grad(r_src, f_src, r_trg, eta)

    def stresslet_normal_density_grad(self, r_src, normals, density, r_trg, eta):
        f_dl = 2.0 * eta * np.einsum("ni,nj->nij", normals, density).reshape(-1, 9)
        return np_stresslet_grad(r_src, f_dl, r_trg, eta)

    def rotlet_grad(self, centers, torques, r_trg, eta):
        return np_rotlet_grad(centers, r_trg, torques, eta)

    def oseen_contract_grad(self, r_src, r_trg, density, eta):
        return np_oseen_grad(r_src, r_trg, density, eta)


# ---- frames from the committed fixtures ----------------------------------

def bent_fiber_frame():
    """Last frame of the committed fiber trajectory. Its two fibers are
    straight and force-free (field ~1e-15), so they are bent here, which
    gives them bending forces; every other field of the frame is as
    recorded."""
    from skellysim_amd.listener import Trajectory
    traj = Trajectory(os.path.join(GOLDEN, "trajectory_fibers.out"))
    for frame in traj.frames:
        for k, fm in enumerate(frame["fibers"][1]):
            x = np.asarray(fm["x_"], float).reshape(-1, 3).copy()
            s = np.linspace(0.0, 1.0, len(x))
            x[:, 0] += 0.15 * np.sin(2 * np.pi * s)
            x[:, 1] += 0.05 * (k + 1) * np.sin(np.pi * s)
            fm["x_"] = x
    return traj


def shell_fixture():
    fx = np.load(os.path.join(GOLDEN, "periphery_sphere_192.npz"))
    return fx, {"nodes": fx["nodes"], "normals": fx["normals"]}


def body_fixture():
    from skellysim_amd.listener import Trajectory
    fx = np.load(os.path.join(GOLDEN, "periphery_sphere_192.npz"))
    geom = {"nodes": fx["nodes"], "normals": -fx["normals"],
            "weights": fx["quadrature_weights"].reshape(-1)}
    traj = Trajectory(os.path.join(GOLDEN, "trajectory_body.out"))
    return traj.frames[0], geom


def far_probes(source_pts, n, seed, box=2.5, clearance=0.5):
    """n points of [-box, box]^3 at least `clearance` from every source."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = rng.uniform(-box, box, 3)
        if np.linalg.norm(source_pts - p, axis=1).min() >= clearance:
            out.append(p)
    return np.array(out)


def fiber_nodes(frame):
    return np.concatenate([np.asarray(fm["x_"], float).reshape(-1, 3)
                           for fm in frame["fibers"][1]])


def assert_gradient_matches_differences(frame, probes, compute, **kw):
    """velocity_gradient_field against central differences of velocity_field,
    h = 1e-5, gate 1e-6 (truncation ~ 10 (h/r)^2 = 4e-9 at r = 0.5)."""
    from skellysim_amd.listener import velocity_field, velocity_gradient_field
    G = velocity_gradient_field(frame, probes, 1.0, compute, **kw)
    assert G.shape == (len(probes), 3, 3)
    fd = central_difference(lambda p: velocity_field(frame, p, 1.0, compute, **kw), probes)
    err = rel(G, fd)
    print("gradient vs central differences:", err)
    assert np.linalg.norm(fd) > 0
    assert err < 1e-6, err
    return G


# ---- the closed forms themselves -----------------------------------------

def test_closed_form_velocities_match_oracle(oracle_mod, golden_dir):
    """The numpy velocity forms are the kernels the oracle pins (so the
    gradient forms differentiate the right fields)."""
    fx = np.load(os.path.join(golden_dir, "refpy_small.npz"))
    eta = float(fx["eta"])
    src, trg = fx["r_src"], fx["r_trg"]
    assert rel(np_stokeslet(src, fx["f3"], trg, eta), fx["u_stokeslet"]) < 1e-12
    assert rel(np_stresslet(src, fx["f9"], trg, eta), fx["u_stresslet"]) < 1e-12
    assert rel(np_oseen(src, trg, fx["f3"], eta), fx["u_oseen"]) < 1e-12
    assert rel(np_rotlet(src, trg, fx["rho"], eta), fx["u_rotlet"]) < 1e-12
    near = fx["near_trg"]
    assert rel(np_oseen(src[:40], near, fx["f3"][:40], eta),
               oracle_mod.oseen_contract(src[:40], near, fx["f3"][:40], eta)) < 1e-12


def test_closed_form_gradients_match_differences():
    rng = np.random.default_rng(3)
    src = rng.uniform(-1, 1, (37, 3))
    f3, f9 = rng.uniform(-1, 1, (37, 3)), rng.uniform(-1, 1, (37, 9))
    u = rng.normal(size=(16, 3))
    trg = 2.5 * u / np.linalg.norm(u, axis=1)[:, None]
    eta = 1.3
    cases = [
        (np_stokeslet_grad(src, f3, trg, eta), lambda p: np_stokeslet(src, f3, p, eta)),
        (np_stresslet_grad(src, f9, trg, eta), lambda p: np_stresslet(src, f9, p, eta)),
        (np_oseen_grad(src, trg, f3, eta), lambda p: np_oseen(src, p, f3, eta)),
        (np_rotlet_grad(src, trg, f3, eta), lambda p: np_rotlet(src, p, f3, eta)),
    ]
    for G, field in cases:
        assert rel(G, central_difference(field, trg)) < 1e-8
        assert np.abs(np.trace(G, axis1=1, axis2=2)).max() < 1e-12 * np.linalg.norm(G)


# ---- velocity_gradient_field ---------------------------------------------

def test_gradient_field_fibers_only():
    frame = bent_fiber_frame().frames[-1]
    probes = far_probes(fiber_nodes(frame), 12, seed=1)
    assert_gradient_matches_differences(frame, probes, NumpyBackend())


def test_gradient_field_with_shell():
    frame = bent_fiber_frame().frames[-1]
    fx, geom = shell_fixture()
    frame["shell"] = {"solution_vec_": np.asarray(fx["density"], float).reshape(-1)}
    probes = far_probes(np.concatenate([fiber_nodes(frame), fx["nodes"]]), 12, seed=2)
    compute = NumpyBackend()
    G = assert_gradient_matches_differences(frame, probes, compute, shell_geometry=geom)
    from skellysim_amd.listener import velocity_gradient_field
    G_fib = velocity_gradient_field(frame, probes, 1.0, compute)
    assert rel(G, G_fib) > 1e-3  # the shell term really takes part


def test_gradient_field_with_body():
    frame, geom = body_fixture()
    from skellysim_amd.listener import bodies_from_frame, velocity_gradient_field
    (b,) = bodies_from_frame(frame, geom)
    assert np.linalg.norm(b.angular_velocity) > 0
    outside = far_probes(b.nodes, 10, seed=3)
    inside = b.position + np.array([0.3, 0.1, 0.0])
    assert np.linalg.norm(inside - b.position) < b.radius
    probes = np.concatenate([outside, inside[None]])
    G = assert_gradient_matches_differences(frame, probes, NumpyBackend(),
                                            body_geometry=geom)
    # inside the body: G_ij = eps_ikj omega_k exactly
    assert np.array_equal(G[-1], np.einsum("ikj,k->ij", EPS, b.angular_velocity))
    assert np.array_equal(curl(G[-1]), 2 * b.angular_velocity)
    G_out = velocity_gradient_field(frame, outside, 1.0, NumpyBackend(), body_geometry=geom)
    assert np.array_equal(G_out, G[:-1])


def test_gradient_field_with_sources():
    from skellysim_amd.sources import PointSource, PointSourceContainer, BackgroundSource
    frame = bent_fiber_frame().frames[-1]
    psc = PointSourceContainer([
        PointSource(position=(0.4, -0.3, 0.2), force=(0.3, -0.1, 0.2)),
        PointSource(position=(-0.5, 0.2, 0.6), torque=(0.0, 0.4, -0.2)),
        PointSource(position=(0.0, 0.9, -0.4), force=(9.0, 9.0, 9.0), time_to_live=0.05),
    ])
    bs = BackgroundSource(components=(1, 2, 0), scale_factor=(0.3, -0.2, 0.1),
                          uniform=(0.05, 0.0, -0.02))
    pts = np.concatenate([fiber_nodes(frame)] + [p.position[None] for p in psc.points])
    probes = far_probes(pts, 12, seed=4)
    compute = NumpyBackend()
    G = assert_gradient_matches_differences(frame, probes, compute, sources=(psc, bs))
    from skellysim_amd.listener import velocity_gradient_field
    G_bare = velocity_gradient_field(frame, probes, 1.0, compute)
    extra = psc.flow_grad(probes, 1.0, float(frame["time"]), compute) + bs.flow_grad(probes)
    assert np.allclose(G - G_bare, extra, rtol=0, atol=1e-14)
    assert np.linalg.norm(extra) > 0.1


# ---- sources --------------------------------------------------------------

def test_background_source_flow_grad():
    from skellysim_amd.sources import BackgroundSource
    bs = BackgroundSource(components=(1, 2, 0), scale_factor=(0.3, -0.2, 0.1),
                          uniform=(0.05, 0.0, -0.02))
    pts = np.random.default_rng(0).uniform(-1, 1, (5, 3))
    G = bs.flow_grad(pts)
    want = np.zeros((3, 3))
    want[0, 1], want[1, 2], want[2, 0] = 0.3, -0.2, 0.1
    assert G.shape == (5, 3, 3) and np.array_equal(G, np.broadcast_to(want, (5, 3, 3)))
    # the affine field's differences are exact up to roundoff
    assert np.allclose(central_difference(bs.flow, pts), G, rtol=0, atol=1e-10)


def test_point_source_flow_grad_liveness():
    from skellysim_amd.sources import PointSource, PointSourceContainer
    always = PointSource(position=(0.1, 0.2, 0.3), force=(1.0, 0.0, -0.5),
                         torque=(0.0, 0.2, 0.0))
    mortal = PointSource(position=(-0.4, 0.0, 0.1), force=(0.0, 2.0, 0.0), time_to_live=1.0)
    psc = PointSourceContainer([always, mortal])
    compute = NumpyBackend()
    pts = far_probes(np.stack([always.position, mortal.position]), 6, seed=5)

    def want(points):
        G = np.zeros((len(pts), 3, 3))
        for p in points:
            if p.force.any():
                G += np_oseen_grad(p.position[None], pts, p.force[None], 1.3)
            if p.torque.any():
                G += np_rotlet_grad(p.position[None], pts, p.torque[None], 1.3)
        return G

    early = psc.flow_grad(pts, 1.3, 0.5, compute)
    late = psc.flow_grad(pts, 1.3, 1.0, compute)  # time >= time_to_live: expired
    assert early.shape == (6, 3, 3)
    assert np.allclose(early, want([always, mortal]), rtol=1e-13, atol=0)
    assert np.allclose(late, want([always]), rtol=1e-13, atol=0)
    assert rel(early, late) > 1e-2
    for t in (0.5, 1.0):
        fd = central_difference(lambda p: psc.flow(p, 1.3, t, compute), pts)
        assert rel(psc.flow_grad(pts, 1.3, t, compute), fd) < 1e-6
    assert not PointSourceContainer([]).flow_grad(pts, 1.3, 0.0, compute).any()


# ---- serve() --------------------------------------------------------------

def _ndencode(obj):
    if isinstance(obj, np.ndarray):
        return ["__eigen__", obj.shape[1], obj.shape[0]] + obj.ravel().tolist()
    return obj


SEED = np.array([[0.9, 0.5, 0.4]])
FIELD_X = np.array([[0.8, 0.6, 0.5], [-0.7, 0.9, 0.2], [0.6, -0.8, 1.4]])


def _request(vortex_extra=None, gradient_x=None):
    cmd = {
        "frame_no": 1,
        "evaluator": "GPU",
        "streamlines": {"dt_init": 0.05, "t_final": 0.1, "abs_err": 1e-10,
                        "rel_err": 1e-8, "back_integrate": False, "x0": SEED},
        "vortexlines": {"dt_init": 0.05, "t_final": 0.1, "abs_err": 1e-10,
                        "rel_err": 1e-8, "back_integrate": False, "x0": SEED},
        "velocity_field": {"x": FIELD_X},
    }
    cmd["vortexlines"].update(vortex_extra or {})
    if gradient_x is not None:
        cmd["velocity_gradient"] = {"x": gradient_x}
    msg = msgpack.packb(cmd, default=_ndencode)
    return struct.pack("<Q", len(msg)) + msg


def _serve(traj, request, compute):
    from skellysim_amd.listener import serve
    stdin = io.BytesIO(request + struct.pack("<Q", 0))
    stdout = io.BytesIO()
    serve(stdin, stdout, traj, compute, eta=1.0)
    raw = stdout.getvalue()
    (size,) = struct.unpack("<Q", raw[:8])
    assert len(raw) == 8 + size
    return raw, msgpack.unpackb(raw[8:], raw=False)


def test_serve_default_path_never_calls_gradients():
    """Without the extension keys the response is, byte for byte, what a
    backend with no gradient methods gives."""
    traj = bent_fiber_frame()
    raw_plain, res_plain = _serve(traj, _request(), NumpyVelocityBackend())
    raw_full, res_full = _serve(traj, _request(), NumpyBackend())
    assert list(res_full.keys()) == ["time", "i_frame", "n_frames", "streamlines",
                                     "vortexlines", "velocity_field"]
    assert raw_full == raw_plain
    # "analytic": false is the same path
    raw_false, _ = _serve(traj, _request({"analytic": False}), NumpyVelocityBackend())
    assert msgpack.unpackb(raw_false[8:], raw=False) == res_plain
    # ... and the extensions do need the gradient methods
    with pytest.raises(AttributeError):
        _serve(traj, _request({"analytic": True}), NumpyVelocityBackend())


def test_serve_analytic_vortexline_and_gradient_block():
    from skellysim_amd.listener import (eigen_decode, velocity_field, velocity_gradient_field,
                                        vorticity)
    traj = bent_fiber_frame()
    compute = NumpyBackend()
    frame = traj.frames[1]
    _, res_fd = _serve(traj, _request(), compute)
    _, res = _serve(traj, _request({"analytic": True}, gradient_x=FIELD_X), compute)
    assert list(res.keys()) == list(res_fd.keys()) + ["velocity_gradient"]
    assert res["streamlines"] == res_fd["streamlines"]
    assert res["velocity_field"] == res_fd["velocity_field"]

    (vl,) = res["vortexlines"]
    x, val = eigen_decode(vl["x"]), eigen_decode(vl["val"])
    assert x.shape == val.shape and x.shape[1] == 3 and len(x) > 2
    w = curl(velocity_gradient_field(frame, x, 1.0, compute))
    assert rel(val, w) < 1e-10
    w_fd = vorticity(lambda p: velocity_field(frame, p, 1.0, compute), x)
    assert rel(w_fd, w) < 1e-6
    # the finite-difference line starts along the same curl
    (vl_fd,) = res_fd["vortexlines"]
    assert rel(eigen_decode(vl_fd["val"])[0], val[0]) < 1e-6

    g = res["velocity_gradient"]
    assert g[:3] == ["__eigen__", 9, len(FIELD_X)]
    block = eigen_decode(g)
    assert block.shape == (9, len(FIELD_X))
    G = velocity_gradient_field(frame, FIELD_X, 1.0, compute)
    assert np.array_equal(block.T.reshape(-1, 3, 3), G)
    fd = central_difference(lambda p: velocity_field(frame, p, 1.0, compute), FIELD_X)
    assert rel(G, fd) < 1e-6


def test_flows_gradient_helpers():
    from skellysim_amd.flows import vorticity_from_gradient, strain_rate_from_gradient
    import torch
    G = np.random.default_rng(1).normal(size=(4, 3, 3))
    assert np.array_equal(vorticity_from_gradient(G), curl(G))
    E = strain_rate_from_gradient(G)
    assert np.array_equal(E, 0.5 * (G + G.transpose(0, 2, 1)))
    Gt = torch.from_numpy(G)
    assert np.array_equal(vorticity_from_gradient(Gt).numpy(), curl(G))
    assert np.array_equal(strain_rate_from_gradient(Gt).numpy(), E)
    # rigid rotation u = Om x r: G_ij = eps_ikj Om_k, curl 2 Om, no strain
    Om = np.array([0.3, -0.7, 0.5])
    R = np.einsum("ikj,k->ij", EPS, Om)
    assert np.array_equal(vorticity_from_gradient(R), 2 * Om)
    assert not strain_rate_from_gradient(R).any()
